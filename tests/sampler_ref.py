"""The built-in sampling draw of the selection kernels (csrc/swx_decode.h: sampler_word, sampler_variate), stated in numpy.

The draw of a row at temperature T > 0 is argmax_i(logits_i / T + g), g one Gumbel variate per (seed, row_uid, step, id):

* the hash word    h = hash32(hash32(lo ^ hash32(id + 0x9e3779b9 * (step + 1))) ^ hash32(row_uid * 0x85ebca6b + hi)) in uint32
  arithmetic, lo / hi the halves of the 64-bit seed; row_uid = uid * 0x9E3779B1 + slot (mod 2^32) with window uids, the row's
  index in the job without;
* the contract of the variate, by bucket k = h >> 8 (float64, every step exact or correctly rounded by numpy):
      u_k = (k + 0.5) * 2^-24        the centre of the bucket, in (0, 1) for every k
      q_k = -ln u_k                  the Exp(1) variate -- the quantity cfg.noise carries
      g_k = -ln q_k                  the Gumbel variate, finite for every k: -2.86 (k = 0) .. 17.33 (k = 2^24 - 1)

``variate_f32`` restates the kernel's OWN arithmetic (f32 throughout, as the device computes it) -- used to measure what f32 costs
against the contract, never as an expectation of a test.

Plain helper module (numpy only, no GPU, no fixtures, not a conftest).
"""
import numpy as np

N_BUCKETS = 1 << 24
UID_MUL = 0x9E3779B1
_M32 = np.uint64(0xFFFFFFFF)


def _u32(x):
    """any integer array-like, reduced mod 2^32, as uint32 (python ints beyond int64 included)"""
    if isinstance(x, np.ndarray):
        if x.dtype == np.uint32:
            return x
        return (x.astype(np.uint64) & _M32).astype(np.uint32)
    if isinstance(x, (int, np.integer)):
        return np.uint32(int(x) & 0xFFFFFFFF)
    return np.array([int(v) & 0xFFFFFFFF for v in x], np.uint32)


def hash32(x):
    x = _u32(x)
    with np.errstate(over="ignore"):
        x = x ^ (x >> np.uint32(16))
        x = x * np.uint32(0x7FEB352D)
        x = x ^ (x >> np.uint32(15))
        x = x * np.uint32(0x846CA68B)
        x = x ^ (x >> np.uint32(16))
    return x


def _unxorshift(x, s):
    y = x
    for _ in range(32 // s + 1):
        y = x ^ (y >> np.uint32(s))
    return y


def hash32_inverse(y):
    """the algebraic inverse of hash32: xor-shifts undone by iteration, the odd multipliers by their inverses mod 2^32"""
    y = _u32(y)
    with np.errstate(over="ignore"):
        y = _unxorshift(y, 16)
        y = y * np.uint32(pow(0x846CA68B, -1, 1 << 32))
        y = _unxorshift(y, 15)
        y = y * np.uint32(pow(0x7FEB352D, -1, 1 << 32))
        y = _unxorshift(y, 16)
    return y


def row_uid(uid, slot):
    """the identity a row draws under when the job carries window uids: uid * 0x9E3779B1 + slot (mod 2^32)"""
    with np.errstate(over="ignore"):
        return _u32(uid) * np.uint32(UID_MUL) + _u32(slot)


def row_uids(W, G, window_uid=None):
    """uint32 [W * G]: the row_uid of every row of a job (row r = window r // G, slot r % G)"""
    r = np.arange(W * G)
    if window_uid is None:
        return r.astype(np.uint32)
    return row_uid(np.asarray(window_uid, np.int64)[r // G], r % G)


def seed_halves(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)


def words_halves(lo, hi, ruid, step, idx):
    """the hash word from the seed's halves given apart; every argument broadcasts"""
    with np.errstate(over="ignore"):
        a = hash32(_u32(lo) ^ hash32(_u32(idx) + np.uint32(0x9E3779B9) * (_u32(step) + np.uint32(1))))
        b = hash32(_u32(ruid) * np.uint32(0x85EBCA6B) + _u32(hi))
    return hash32(a ^ b)


def words(seed, ruid, step, idx):
    """h(seed, row_uid, step, id), uint32; ruid / step / idx broadcast against one another"""
    lo, hi = seed_halves(seed)
    return words_halves(lo, hi, ruid, step, idx)


def bucket(h):
    return _u32(h) >> np.uint32(8)


def u_of_bucket(k):
    return (np.asarray(k, np.float64) + 0.5) * 2.0 ** -24          # exact: k + 0.5 has 25 bits


def q_of_bucket(k):
    return -np.log(u_of_bucket(k))


def g_of_bucket(k):
    return -np.log(q_of_bucket(k))


def variate_f32(k):
    """the kernel's word-to-variate map restated in numpy float32, operation by operation: k + 0.5f rounds to even from 2^23 on
    (k odd -> k + 1) and would reach 1.0f in the top bucket, where it is held at the largest f32 below 1"""
    k = np.asarray(k)
    u = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))
    return -np.log(-np.log(u, dtype=np.float32), dtype=np.float32)


def central(k):
    """the buckets the accuracy condition is stated on: 2^-12 <= u_k <= 1 - 2^-12"""
    u = u_of_bucket(k)
    return (u >= 2.0 ** -12) & (u <= 1.0 - 2.0 ** -12)


def job_words(seed, S, W, G, V, window_uid=None):
    """uint32 [S][W * G][V]: the word of every (step, row, id) of a job"""
    ru = row_uids(W, G, window_uid)
    return words(seed, ru[None, :, None], np.arange(S, dtype=np.uint32)[:, None, None], np.arange(V, dtype=np.uint32)[None, None, :])


def job_q(seed, S, W, G, V, window_uid=None):
    """float64 [S][W * G][V]: the Exp(1) variates q of a job -- what a scripted case feeds the reference in place of cfg.noise
    while the device draws with noise = NULL"""
    return q_of_bucket(bucket(job_words(seed, S, W, G, V, window_uid)))


def find_top_bucket(S, W, G, V, max_step, seeds, window_uid=None, hi=0x5bd1e995):
    """the first seed (hi << 32 | s, s in `seeds`) under which some (step <= max_step, row, id) of the job lands in the top
    bucket: (seed, step, row, id), or None"""
    for s in seeds:
        seed = (hi << 32) | int(s)
        h = job_words(seed, min(S, max_step + 1), W, G, V, window_uid)
        hit = np.argwhere(bucket(h) == N_BUCKETS - 1)
        if len(hit):
            step, row, idx = (int(v) for v in hit[0])
            return seed, step, row, idx
    return None
