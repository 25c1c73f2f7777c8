"""The built-in sampling draw of the selection kernels (csrc/swx_decode.h: sampler_word, sampler_variate -- what decode_select_kernel
and decode_select_reg_kernel add to logits / T when cfg.noise is NULL) against its float64 statement, tests/sampler_ref.py.

* the hash words are exact (swx_test_sampler_words), edges of every coordinate included;
* all 2^24 variates from one launch (swx_test_sampler_buckets): finite, non-decreasing, never more than one bucket off, and on
  the central buckets (2^-12 <= u_k <= 1 - 2^-12) within `tol` of g_k.  tol = 4 x the error a numpy-float32 restatement of the
  same arithmetic has against float64 on those buckets (measured here on the CPU, 1.22e-4: it is the rounding of k + 0.5f from
  bucket 2^23 on, which the two logarithms near u = 1 magnify; the factor allows the device library's logf a couple of ulp more
  than numpy's) -- profiles/sampler_variate_error.json keeps the figures;
* the uid keying of the draw through swx_test_decode_script: a window draws the same alone and in company, and two windows that
  trade uids trade draws.

The statistical quality of the stream is a property of the integer hash and is proved on the CPU (tests/test_sampler_ref_cpu.py);
the scripted cases that run the draw through both selection kernels (hashed_*, top_bucket_*) are in tests/select_script.py.
"""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import sampler_ref as sr
import select_script as ss
from test_gpu_select_script import run_gpu

pytestmark = pytest.mark.gpu

V_REAL = 51866
M64 = (1 << 64) - 1


def _lib():
    from stable_ts_amd import _lib as L
    return L.load()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_words(seed, ruid, step, id0, n):
    words = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    var = torch.full((n,), float("nan"), device="cuda:0")
    rc = _lib().swx_test_sampler_words(seed, ruid, step, id0, n, ctypes.c_void_p(words.data_ptr()), ctypes.c_void_p(var.data_ptr()),
                                       _stream())
    assert rc == 0
    torch.cuda.synchronize()
    return words.cpu().numpy().view(np.uint32), var.cpu().numpy()


SEEDS = [0, M64, 0x00000000DEADBEEF, 0x9E3779B900000000, 0x5BD1E99500000001]
ROW_UIDS = [0, 1, (1 << 32) - 1, int(sr.row_uid(3_000_000, 2))]


@pytest.mark.parametrize("seed", SEEDS, ids=["zero", "ones", "low_only", "high_only", "both"])
def test_words_are_exact(seed):
    """4 row uids x 2 steps x (1024 + 1024) ids per seed, the first and the last id of a V = 51866 row among them; and the variate
    the hook reports beside a word is the bucket map applied to that word, bit for bit"""
    lib = _lib()
    n = 1024
    for ruid in ROW_UIDS:
        for step in (0, 447):
            for id0 in (0, V_REAL - n):
                got, var = _device_words(seed, ruid, step, id0, n)
                want = sr.words(seed, ruid, step, np.arange(id0, id0 + n))
                assert (got == want).all(), (hex(seed), ruid, step, id0, np.flatnonzero(got != want)[:4])
    one = torch.full((1,), float("nan"), device="cuda:0")
    for j in (0, 1, n // 2, n - 1):
        assert lib.swx_test_sampler_buckets(int(got[j] >> 8), 1, ctypes.c_void_p(one.data_ptr()), _stream()) == 0
        torch.cuda.synchronize()
        assert one.cpu().numpy().view(np.uint32)[0] == var.view(np.uint32)[j]


def test_the_issue_table_of_top_bucket_tuples():
    """(seed, row, step, id) of a V = 51866 job whose word lies in the top bucket: the device's words say so too, and the variate
    the kernels use there is finite"""
    for seed, row, step, idx in ((0, 1, 37, 3905), (0, 3, 69, 30905), (1, 0, 157, 15165)):
        got, var = _device_words(seed, row, step, idx, 1)
        assert got[0] >> 8 == sr.N_BUCKETS - 1 and got[0] == sr.words(seed, row, step, idx)
        assert np.isfinite(var[0]), (seed, row, step, idx, var[0])


@pytest.fixture(scope="module")
def contract():
    """g_k of all 2^24 buckets (float64), the central mask, and the measured error of the numpy-float32 restatement there"""
    k = np.arange(sr.N_BUCKETS)
    g = sr.g_of_bucket(k)
    c = sr.central(k)
    cpu_err = float(np.abs(sr.variate_f32(k).astype(np.float64) - g)[c].max())
    return g, c, cpu_err


def test_every_bucket(contract):
    g, c, cpu_err = contract
    tol = 4.0 * cpu_err
    n = sr.N_BUCKETS
    out = torch.full((n,), float("nan"), device="cuda:0")
    assert _lib().swx_test_sampler_buckets(0, n, ctypes.c_void_p(out.data_ptr()), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    bad = np.flatnonzero(~np.isfinite(got))
    err = np.abs(got - g)
    with np.errstate(invalid="ignore"):
        print(f"cpu f32 restatement: max central error {cpu_err:.6e}; tol {tol:.6e}; device: max central error {np.nanmax(err[c]):.6e} "
              f"at k = {int(np.nanargmax(np.where(c, err, -1.0)))}; got[0] = {got[0]!r}, got[-2:] = {got[-2:].tolist()}; "
              f"non-finite at k = {bad[:4].tolist()} ({got[bad[:4]].tolist()})")
    assert bad.size == 0, (bad[:4].tolist(), got[bad[:4]].tolist())
    d = np.diff(got)
    assert (d >= 0).all(), (np.flatnonzero(d < 0)[:4].tolist(),)
    lo = np.concatenate([g[:1], g[:-1]]) - tol          # g_{k-1} - tol, the end value itself at k = 0
    hi = np.concatenate([g[1:], g[-1:]]) + tol          # g_{k+1} + tol, the end value itself at k = 2^24 - 1
    off = np.flatnonzero((got < lo) | (got > hi))
    assert off.size == 0, (off[:4].tolist(), got[off[:4]].tolist(), g[off[:4]].tolist())
    worst = np.flatnonzero(c & ~(err <= tol))
    assert worst.size == 0, (worst[:4].tolist(), err[worst[:4]].tolist(), tol)


def test_bucket_hook_ranges():
    """the hook writes [k0, k0 + n) and nothing else, up to the last bucket, and refuses a range outside [0, 2^24)"""
    lib = _lib()
    out = torch.full((1000,), -7.0, device="cuda:0")
    k0 = sr.N_BUCKETS - 700
    assert lib.swx_test_sampler_buckets(k0, 700, ctypes.c_void_p(out.data_ptr()), _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[700:] == -7.0).all() and np.isfinite(got[:700]).all()
    assert np.abs(got[:600].astype(np.float64) - sr.g_of_bucket(np.arange(k0, k0 + 600))).max() < 0.5
    assert lib.swx_test_sampler_buckets(k0, 701, ctypes.c_void_p(out.data_ptr()), _stream()) < 0
    assert lib.swx_test_sampler_buckets(-1, 4, ctypes.c_void_p(out.data_ptr()), _stream()) < 0


# ------------------------------------------------------------------------------------------------------------- uid keying
UID_A, UID_B = ss.UIDS


def _twin(window_uid):
    """the hashed T = 1 case at V = 1601 with BOTH windows on window 0's rows: what differs between them is the uid alone"""
    c = ss.case_hashed_sampling(1601, 1.0, window_uid)
    G = c.G
    c.prefill[1] = c.prefill[0]
    c.script[:, G:2 * G] = c.script[:, :G]
    return c


def _window(case, w):
    """window w of a case as a job of its own"""
    G = case.G
    return dataclasses.replace(case, name=f"{case.name}_w{w}", W=1, init=[case.init[w]], prefill=case.prefill[w:w + 1].copy(),
                               script=case.script[:, w * G:(w + 1) * G].copy(), window_uid=(case.window_uid[w],), _q=None)


def _same_as_reference(got, ref, name):
    used = ref.lens >= 0
    assert got["lens"].tolist() == ref.lens.tolist(), name
    assert got["tokens"][used].tolist() == ref.tokens[used].tolist(), name
    assert got["steps"] == ref.steps and got["pos0"].tolist() == ref.pos0.tolist(), name
    assert (np.abs(got["sumlp"][used] - ref.sumlp[used]) <= 1e-4).all(), (name, got["sumlp"], ref.sumlp)


@pytest.mark.parametrize("mem_kernel", [0, 1], ids=["reg", "mem"])
def test_uid_keys_the_draw(mem_kernel):
    ab, ba = _twin((UID_A, UID_B)), _twin((UID_B, UID_A))
    alone = _window(ab, 1)
    refs = {c.name + str(c.window_uid): ss.run_reference(c) for c in (ab, ba, alone)}
    for r in refs.values():
        assert min(m[3] for m in r.margins) >= ss.MARGIN
    r_ab, r_ba, r_alone = refs.values()
    # the reference itself: keyed on uid * 0x9E3779B1 + slot, window B draws what it draws alone, and not what window A draws
    assert r_ab.tokens[1].tolist() == r_alone.tokens[0].tolist() and r_ab.tokens[0].tolist() != r_ab.tokens[1].tolist()
    g_ab, g_ba, g_alone = run_gpu(ab, mem_kernel), run_gpu(ba, mem_kernel), run_gpu(alone, mem_kernel)
    _same_as_reference(g_ab, r_ab, "ab")
    _same_as_reference(g_ba, r_ba, "ba")
    _same_as_reference(g_alone, r_alone, "alone")
    # uid B's three sequences: identical in company and alone (the job's shortest window decides `steps`, not the tokens)
    assert g_ab["tokens"][1].tolist() == g_alone["tokens"][0].tolist() and g_ab["lens"][1].tolist() == g_alone["lens"][0].tolist()
    assert (g_ab["sumlp"][1] == g_alone["sumlp"][0]).all()
    # trading uids trades the draws
    assert g_ba["tokens"][0].tolist() == g_ab["tokens"][1].tolist() and g_ba["tokens"][1].tolist() == g_ab["tokens"][0].tolist()
    assert (g_ba["sumlp"][::-1] == g_ab["sumlp"]).all()


def test_null_uids_key_on_the_row():
    """window_uid = NULL behaves as before: row r draws under row_uid = r, so window 1 of a job does NOT draw what it draws alone"""
    c = _twin(None)
    ref = ss.run_reference(c)
    assert min(m[3] for m in ref.margins) >= ss.MARGIN
    got = run_gpu(c, 0)
    _same_as_reference(got, ref, c.name)
    assert got["tokens"][0].tolist() != got["tokens"][1].tolist()
