"""The hashed sampling draw as stated in tests/sampler_ref.py, on the CPU alone: the quality of the stream is a property of
integer arithmetic, so it is proved here, at scale, and the GPU tests (tests/test_gpu_sampler.py) only tie the device to the
statement bit for bit.

Every statistical test is a CONDITION: its chi-square statistic lies below the 1 - 1e-6 quantile of its null distribution.  The
input is deterministic, so a pass is permanent.  Each runs a second time with numpy's PCG64(0) supplying the 32-bit words in place
of the hash (`source` = "pcg64"): the same picks, tables and thresholds on a generator of known quality, so the thresholds are
visibly not tuned to the hash.

Also here: hash32 is a bijection (its algebraic inverse), the statement reproduces known top-bucket tuples, the hash inputs do
not collide at production extents, the numpy-float32 restatement of the kernel's arithmetic meets the conditions the GPU test puts
to the device (and the arithmetic before the top bucket was held below 1 does not), and profiles/sampler_variate_error.json holds
what is measured here.
"""
import json
import os

import numpy as np
import pytest

import sampler_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_TAIL = 1e-6
SOURCES = ["hash", "pcg64"]
SEED = 0x5BD1E995_0000002A
LO, HI = sr.seed_halves(SEED)
V, STEPS = 51866, 448


def _quantile(df):
    from scipy.stats import chi2
    return float(chi2.ppf(1.0 - P_TAIL, df))


def _words(source, shape, lo=LO, hi=HI, ruid=5, step=3, idx=11):
    """uint32 words of `shape`: the hash of the (broadcast) coordinates, or as many words of PCG64(0)"""
    if source == "pcg64":
        return np.random.Generator(np.random.PCG64(0)).integers(0, 1 << 32, size=shape, dtype=np.uint32)
    return np.broadcast_to(sr.words_halves(lo, hi, ruid, step, idx), shape)


def _gof(counts, p):
    n = counts.sum()
    return float((((counts - n * p) ** 2) / (n * p)).sum())


def _independence(a, b, n_cat):
    """Pearson's statistic of the n_cat x n_cat contingency table of paired picks against the product of its margins"""
    t = np.bincount(a * n_cat + b, minlength=n_cat * n_cat).reshape(n_cat, n_cat).astype(np.float64)
    e = np.outer(t.sum(1), t.sum(0)) / t.sum()
    assert e.min() >= 100, e.min()
    return float(((t - e) ** 2 / e).sum())


def _picks(words, logits, T):
    """Gumbel-max over the last axis: argmax_i(logits_i / T + g(bucket of word i)), the contract's float64 variates"""
    return np.argmax(np.asarray(logits, np.float64) / T + sr.g_of_bucket(sr.bucket(words)), axis=-1)


# ------------------------------------------------------------------------------------------------------- the statement itself
def test_hash32_is_a_bijection():
    """both multipliers are odd and every xor-shift is undone by iteration: hash32_inverse is a two-sided inverse -- on the
    edges, on 2^22 inputs strided over the whole range and on 2^22 consecutive ones"""
    assert 0x7FEB352D % 2 == 1 and 0x846CA68B % 2 == 1
    stride = np.arange(1 << 22, dtype=np.uint64) * np.uint64(1021) + np.uint64(7)
    xs = np.concatenate([np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64), stride,
                         np.arange(1 << 22, dtype=np.uint64) + np.uint64(0xFFC00000)]).astype(np.uint32)
    assert int(stride.max()) < 1 << 32 and len(np.unique(xs)) >= 1 << 23
    assert (sr.hash32_inverse(sr.hash32(xs)) == xs).all()
    assert (sr.hash32(sr.hash32_inverse(xs)) == xs).all()
    assert sr.hash32(0) == 0 and len(np.unique(sr.hash32(xs))) == len(np.unique(xs))


def test_known_top_bucket_tuples():
    """(seed, row, step, id) of a V = 51866 job without uids whose word lies in the top bucket"""
    for seed, row, step, idx in ((0, 1, 37, 3905), (0, 3, 69, 30905), (1, 0, 157, 15165)):
        assert sr.bucket(sr.words(seed, row, step, idx)) == sr.N_BUCKETS - 1
    # and the row really is the first such of its job: the helper the scripted cases use finds it
    h = sr.job_words(0, 38, 1, 2, V)
    first = np.argwhere(sr.bucket(h) == sr.N_BUCKETS - 1)
    assert [int(v) for v in first[0]] == [37, 1, 3905]


def test_row_uid_and_seed_halves():
    assert sr.row_uid(0, 3) == 3 and sr.row_uid(1, 0) == 0x9E3779B1 and sr.row_uid(3_000_000, 2) == (3_000_000 * 0x9E3779B1 + 2) % (1 << 32)
    assert sr.row_uids(2, 3).tolist() == [0, 1, 2, 3, 4, 5]
    assert sr.row_uids(2, 3, [7, 9]).tolist() == [(7 * 0x9E3779B1 + s) % (1 << 32) for s in range(3)] + \
        [(9 * 0x9E3779B1 + s) % (1 << 32) for s in range(3)]
    assert sr.seed_halves((0xABCD << 32) | 0x1234) == (0x1234, 0xABCD)
    # the two halves enter at different places: swapping them is another stream
    assert sr.words((1 << 32) | 2, 0, 0, 0) != sr.words((2 << 32) | 1, 0, 0, 0)
    q = sr.job_q(SEED, 2, 2, 3, 100, (7, 9))
    assert q.shape == (2, 6, 100) and q.dtype == np.float64 and (q > 0).all()
    assert q[1, 4, 17] == -np.log((float(sr.words(SEED, sr.row_uid(9, 1), 1, 17) >> 8) + 0.5) / 2 ** 24)


def test_bucket_contract_ends():
    k = np.array([0, 1, (1 << 23) - 1, 1 << 23, sr.N_BUCKETS - 2, sr.N_BUCKETS - 1])
    u = sr.u_of_bucket(k)
    assert u[0] == 2.0 ** -25 and u[-1] == 1.0 - 2.0 ** -25 and (np.diff(u) > 0).all()
    g = sr.g_of_bucket(k)
    assert np.isfinite(g).all() and abs(g[0] + np.log(25 * np.log(2))) < 1e-12 and abs(g[-1] - 25 * np.log(2)) < 1e-7
    assert 17.32 < g[-1] < 17.33 and -2.86 < g[0] < -2.85


# ------------------------------------------------------------------------------------------------------------- uniformity
N_UNIFORM = 1 << 21          # 2 097 152 words >= 2e6


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("vary", ["id", "step", "row_uid", "seed_lo", "seed_hi", "all"])
def test_buckets_are_uniform(vary, source):
    """chi-square of the top 12 bits of the bucket (4096 cells, 512 expected) while ONE coordinate counts up from 0 and the
    others stand still; `all`: every coordinate moves at once, each by an odd stride of its own"""
    i = np.arange(N_UNIFORM, dtype=np.uint64)
    co = dict(lo=LO, hi=HI, ruid=5, step=3, idx=11)
    name = {"id": "idx", "step": "step", "row_uid": "ruid", "seed_lo": "lo", "seed_hi": "hi"}
    if vary == "all":
        for n, (key, mul) in enumerate(zip(("idx", "step", "ruid", "lo", "hi"), (1, 3, 0x9E3779B1, 5, 7))):
            co[key] = sr._u32(i * np.uint64(mul) + np.uint64(n))
    else:
        co[name[vary]] = sr._u32(i)
    h = _words(source, (N_UNIFORM,), **co)
    cells = np.bincount(sr.bucket(h) >> 12, minlength=4096)
    stat = _gof(cells, np.full(4096, 1 / 4096))
    print(vary, source, "chi2 =", stat, "limit", _quantile(4095))
    assert stat < _quantile(4095)


# ----------------------------------------------------------------------------------------------------------- independence
FLAT16 = np.linspace(-0.5, 0.5, 16)        # a fixed 16-way row, probabilities 0.038 .. 0.10 at T = 1: every cell is well filled
N_PAIRS = 1 << 17


def _pair_stat(source, ruid_a, step_a, ruid_b, step_b):
    shape = (2, N_PAIRS, 16)
    idx = np.arange(16, dtype=np.uint32)[None, None, :]
    ruid = np.stack([np.broadcast_to(sr._u32(ruid_a), (N_PAIRS,)), np.broadcast_to(sr._u32(ruid_b), (N_PAIRS,))])[:, :, None]
    step = np.stack([sr._u32(step_a), sr._u32(step_b)])[:, :, None]
    p = _picks(_words(source, shape, ruid=ruid, step=step, idx=idx), FLAT16, 1.0)
    return _independence(p[0], p[1], 16)


@pytest.mark.parametrize("source", SOURCES)
def test_consecutive_steps_are_independent(source):
    """the pick of one row at step 2t against its pick at step 2t + 1: 16 x 16 table, 131072 pairs"""
    t = np.arange(N_PAIRS, dtype=np.int64) * 2
    stat = _pair_stat(source, 5, t, 5, t + 1)
    print(source, "chi2 =", stat, "limit", _quantile(225))
    assert stat < _quantile(225)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("pair", [(0, 1), (3, 4), (0, 7), (6, 7)])
def test_slots_of_a_window_are_independent(pair, source):
    """the picks of two slots of one window (G = 8) at the same step, over 131072 steps"""
    t = np.arange(N_PAIRS, dtype=np.int64)
    uid = 1234567
    stat = _pair_stat(source, sr.row_uid(uid, pair[0]), t, sr.row_uid(uid, pair[1]), t)
    print(pair, source, "chi2 =", stat, "limit", _quantile(225))
    assert stat < _quantile(225)


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("uid", [0, 1234567, 2_999_999])
def test_neighbouring_windows_are_independent(uid, source):
    """slot 0 of window uid against slot 0 of window uid + 1 at the same step"""
    t = np.arange(N_PAIRS, dtype=np.int64)
    stat = _pair_stat(source, sr.row_uid(uid, 0), t, sr.row_uid(uid + 1, 0), t)
    print(uid, source, "chi2 =", stat, "limit", _quantile(225))
    assert stat < _quantile(225)


# -------------------------------------------------------------------------------------------------------- pick frequencies
_MID = np.geomspace(2e-3, 0.1, 14)
P16 = np.concatenate([[1e-3], _MID * (0.499 / _MID.sum()), [0.5]])       # 16-way categorical: 1e-3, a geometric ladder, 0.5
N_DRAWS = 1 << 18                          # 262 144 >= 2e5


def test_the_ladder_spans_what_is_asked():
    assert P16.min() == 1e-3 and P16.max() == 0.5 and abs(P16.sum() - 1.0) < 1e-15 and (np.diff(P16) > 0).all()
    assert (P16 * N_DRAWS).min() > 100


@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("T", [0.2, 1.0])
@pytest.mark.parametrize("walk", ["steps", "rows"])
def test_pick_frequencies_follow_the_softmax(walk, T, source):
    """Gumbel-max picks of logits = T ln p against softmax(logits / T) = p in float64, over the steps of one row / over the
    rows of one step"""
    logits = T * np.log(P16)
    z = logits / T
    p = np.exp(z - z.max()); p /= p.sum()
    assert np.abs(p - P16).max() < 1e-15
    n = np.arange(N_DRAWS, dtype=np.uint32)[:, None]
    idx = (np.arange(16, dtype=np.uint32) * np.uint32(3001) + np.uint32(17))[None, :]       # 16 ids spread over the vocabulary
    co = dict(ruid=5, step=n) if walk == "steps" else dict(ruid=n, step=3)
    picks = _picks(_words(source, (N_DRAWS, 16), idx=idx, **co), logits, T)
    stat = _gof(np.bincount(picks, minlength=16), p)
    print(walk, T, source, "chi2 =", stat, "limit", _quantile(15))
    assert stat < _quantile(15)


# -------------------------------------------------------------------------------------------------------------- collisions
def test_no_collision_of_the_id_step_word():
    """id + 0x9e3779b9 * (step + 1) mod 2^32 is distinct over id < 51866, step < 448 (23.2 million inputs of the inner hash)"""
    with np.errstate(over="ignore"):
        x = (np.arange(V, dtype=np.uint32)[None, :] + np.uint32(0x9E3779B9) * (np.arange(STEPS, dtype=np.uint32)[:, None] + np.uint32(1))).ravel()
    x.sort()
    assert int((x[1:] == x[:-1]).sum()) == 0


def test_no_collision_of_row_uids():
    """uid * 0x9E3779B1 + slot mod 2^32 is distinct over slot < 8, uid = 0 .. 3 000 000 (window uids are seek positions in frames:
    3e6 frames are 8 hours 20 minutes)"""
    x = sr.row_uid(np.arange(3_000_001, dtype=np.int64)[:, None], np.arange(8, dtype=np.int64)[None, :]).ravel()
    x.sort()
    assert int((x[1:] == x[:-1]).sum()) == 0


# ----------------------------------------------------------------------------------------- the f32 arithmetic of the kernel
@pytest.fixture(scope="module")
def f32_survey():
    k = np.arange(sr.N_BUCKETS)
    g = sr.g_of_bucket(k)
    c = sr.central(k)
    f = sr.variate_f32(k).astype(np.float64)
    return k, g, c, f


def test_f32_restatement_meets_the_device_conditions(f32_survey):
    """what tests/test_gpu_sampler.py::test_every_bucket asks of the device, asked of the numpy-float32 restatement -- with the
    tolerance at 1 x its own central error, where the device gets 4 x"""
    k, g, c, f = f32_survey
    tol = float(np.abs(f - g)[c].max())
    assert np.isfinite(f).all() and (np.diff(f) >= 0).all()
    assert (f >= np.concatenate([g[:1], g[:-1]]) - tol).all() and (f <= np.concatenate([g[1:], g[-1:]]) + tol).all()
    # the error is the rounding of k + 0.5f from bucket 2^23 on (half a bucket, 2^-25 of u), magnified by 1 / (1 - u) <= 2^12
    assert 2.0 ** -13 <= tol <= 2.0 ** -13 * 1.01
    low = c & (k < 1 << 23)
    assert np.abs(f - g)[low].max() < 2e-6


def test_arithmetic_without_the_hold_is_not_finite_in_the_top_bucket():
    """(k + 0.5f) * 2^-24f is 1.0f at k = 2^24 - 1 (16777215.5 rounds to even): -log(-log(1)) = +inf.  One bucket in 2^24"""
    k = np.arange(sr.N_BUCKETS - 4, sr.N_BUCKETS)
    u = (k.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert u[-1] == np.float32(1.0) and (u[:-1] < 1.0).all()
    with np.errstate(divide="ignore"):
        raw = -np.log(-np.log(u, dtype=np.float32), dtype=np.float32)
    assert np.isposinf(raw[-1]) and np.isfinite(raw[:-1]).all()
    held = sr.variate_f32(k)
    assert (held[:-1].view(np.uint32) == raw[:-1].view(np.uint32)).all() and np.isfinite(held[-1])


def test_profile_holds_what_is_measured_here(f32_survey):
    k, g, c, f = f32_survey
    prof = json.load(open(os.path.join(ROOT, "profiles", "sampler_variate_error.json")))
    measured = float(np.abs(f - g)[c].max())
    assert abs(prof["cpu_f32_restatement_max_central_error"] - measured) <= 1e-3 * measured
    assert prof["device_bound"] == 4.0 * prof["cpu_f32_restatement_max_central_error"]
    assert prof["central_buckets"] == int(c.sum())
    assert 0 < prof["device_max_central_error"] <= prof["device_bound"]
