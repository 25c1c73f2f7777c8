"""The chunked self-attention K cache (csrc/swx_kernels.h: KLayout -- a cache row as [H][8][n_ctx][8] instead of [n_ctx][d]) against
the row-major one, kernel by kernel: only addresses differ, so every output must be EQUAL, bit for bit.

* readers: the decode-step kernels, the long-context kernels and the multi-token kernels are run on a row-major cache and on its
  re-laid-out copy (swx_test_kcache_relayout, the library's own index function).  Every cache position a row must not read holds
  a NaN, so a load that strays poisons the output and the comparison fails (NaN != NaN).
* writers: the QKV scatter of the dec GEMMs (and kv_append_kernel) into a guard-filled cache: the chunked cache afterwards is the
  re-laid-out row-major one, guard pattern included.
* end to end: transcribe() with the layout switch (swx_debug_flags bit 2 = chunked) on and off.
"""
import ctypes
import json

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D, H, N_CTX, R = 384, 6, 448, 7
GROUPS = ((0, 1, 2, 3), (4, 5, 6))                   # rows that may be each other's ancestors (the beams of two windows)
POSITIONS = (0, 1, 7, 8, 63, 64, 65, 127, 128, 129, 191, 319, 320, 447)     # both sides of every chunk / batch edge of the kernels
FLAG_CHUNKED, FLAG_NO_DEEP, FLAG_DEC_NO_W1 = 2, 4, 16
K_CACHED_F16, K_MQ4, K_MQ8, K_STEP, K_STEP_LONG, K_STEP_DEEP = 0, 2, 3, 4, 6, 8
DEC_W4, DEC_W1, DEC_TALL4 = 0, 1, 2


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy()


def _chunked(lib, cache, n_ctx, d):
    """row-major f16 cache [rows][n_ctx][d] (CPU tensor) -> its chunked copy, through the library's helper"""
    src = np.ascontiguousarray(cache.view(torch.int16).numpy())
    dst = np.zeros_like(src)
    rc = lib.swx_test_kcache_relayout(ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data), src.shape[0], n_ctx, d, 2, 1)
    assert rc == 0, rc
    return torch.from_numpy(dst).view(torch.float16)


def _step_inputs(rng, pos, use_anc, rows=R, heads=H, n_ctx=N_CTX):
    """q, K / V caches (CPU, row-major, NaN wherever no row of the launch may read), ancestor table, positions"""
    d = 64 * heads
    pos = np.asarray(pos, np.int32)
    groups = GROUPS if rows == R else (tuple(range(rows)),)
    anc = np.empty((rows, n_ctx), np.int32)
    for g in groups:
        for r in g:
            anc[r] = rng.choice(g, n_ctx)
            anc[r, pos[r]:] = r                      # the table names the row itself from its newest position on (as the beam bookkeeping leaves it)
    valid = np.zeros((rows, n_ctx), bool)
    for r in range(rows):
        for p in range(pos[r]):
            valid[anc[r, p] if use_anc else r, p] = True
        valid[r, pos[r]] = True                      # the new token's K / V are the row's own
    kv = []
    for _ in range(2):
        c = rng.standard_normal((rows, n_ctx, d)).astype(np.float16)
        c[~valid] = np.float16(np.nan)
        kv.append(torch.from_numpy(c))
    q = torch.from_numpy(rng.standard_normal((rows, d)).astype(np.float16))
    return q, kv[0], kv[1], torch.from_numpy(anc) if use_anc else None, torch.from_numpy(pos)


# (name, kernel id, positions it has, launch): variants 0 / 1 / 2 of swx_test_self_attn_step and the long-context kernel of many waves
# through the general call (step_variant 2 with the two-batch kernel switched off)
STEP_KERNELS = {
    "step": (K_STEP, 127, 0, lambda lib, a, ch: lib.swx_test_self_attn_step_kl(*a[:5], R, H, N_CTX, D, 0, ch, a[5], _stream())),
    "deep": (K_STEP_DEEP, 447, 0, lambda lib, a, ch: lib.swx_test_self_attn_step_kl(*a[:5], R, H, N_CTX, D, 1, ch, a[5], _stream())),
    "cached": (K_CACHED_F16, 447, 0, lambda lib, a, ch: lib.swx_test_self_attn_step_kl(*a[:5], R, H, N_CTX, D, 2, ch, a[5], _stream())),
    "long": (K_STEP_LONG, 447, FLAG_NO_DEEP,
             lambda lib, a, ch: lib.swx_test_self_attn_general_kl(1, a[0], D, a[1], a[2], a[3], a[4], R, H, 1, N_CTX, D, 1, 1, 0, 2, ch, a[5],
                                                                  _stream())),
}


@pytest.mark.parametrize("use_anc", [True, False], ids=["anc", "noanc"])
@pytest.mark.parametrize("kernel", list(STEP_KERNELS))
def test_step_readers_chunked_equals_row_major(kernel, use_anc):
    lib = _lib()
    kid, max_pos, flags, launch = STEP_KERNELS[kernel]
    rng = np.random.default_rng(17 + 2 * list(STEP_KERNELS).index(kernel) + use_anc)
    here = [p for p in POSITIONS if p <= max_pos]
    # every position with all rows on it, then launches whose rows sit on different positions (each position once more)
    launches = [[p] * R for p in here] + [[here[(s + 2 * r) % len(here)] for r in range(R)] for s in (0, 1, 5)]
    old = lib.swx_debug_flags(-1)
    base = old & ~FLAG_NO_DEEP
    try:
        lib.swx_debug_flags(base | flags)
        step_cached = 0 if kernel == "cached" else 1
        assert lib.swx_test_self_attn_plan(1, R, H, 1, N_CTX, 1, 1, step_cached, 128 if kernel == "step" else 0, 0, 1 if use_anc else 0,
                                           base | flags) == kid
        for pos in launches:
            q, kc, vc, anc, p0 = _step_inputs(rng, pos, use_anc)
            kcc = _chunked(lib, kc, N_CTX, D)
            dq, dv, da, dp = q.cuda(), vc.cuda(), None if anc is None else anc.cuda(), p0.cuda()
            outs = []
            for ch, cache in ((0, kc), (1, kcc)):
                dk = cache.cuda()
                o = torch.full((R, D), float("nan"), dtype=torch.half, device="cuda")
                rc = launch(lib, (_p(dq), _p(dk), _p(dv), _p(da), _p(dp), _p(o)), ch)
                torch.cuda.synchronize()
                assert rc == 0, (kernel, pos, ch, rc)
                assert np.array_equal(_bits(dk), _bits(cache))                  # read-only
                outs.append(o.cpu().numpy())
            assert np.isfinite(outs[0]).all(), (kernel, pos)
            assert np.array_equal(outs[0], outs[1]), (kernel, pos)
    finally:
        lib.swx_debug_flags(old)


@pytest.mark.parametrize("heads,rows", [(H, R), (20, 2)])
@pytest.mark.parametrize("n_new", [1, 7, 8, 9, 113])
def test_multi_token_readers_chunked_equals_row_major(n_new, heads, rows):
    lib = _lib()
    d = 64 * heads
    rng = np.random.default_rng(1000 * heads + n_new)
    kv = []
    for _ in range(2):
        c = rng.standard_normal((rows, N_CTX, d)).astype(np.float16)
        c[:, n_new:] = np.float16(np.nan)            # rows start at position 0: token i attends to positions 0 .. i
        kv.append(torch.from_numpy(c))
    kc, vc = kv
    kcc = _chunked(lib, kc, N_CTX, d)
    q = torch.from_numpy(rng.standard_normal((rows * n_new, d)).astype(np.float16)).cuda()
    dv = vc.cuda()
    flags = lib.swx_debug_flags(-1)
    for mq in (0, 1):
        want = K_CACHED_F16 if (mq == 0 or n_new < 8) else K_MQ4 if n_new < 32 else K_MQ8
        assert lib.swx_test_self_attn_plan(1, rows, heads, n_new, N_CTX, 1, 1, 0, 0, mq, 0, flags) == want
        outs = []
        for ch, cache in ((0, kc), (1, kcc)):
            dk = cache.cuda()
            o = torch.full((rows * n_new, d), float("nan"), dtype=torch.half, device="cuda")
            rc = lib.swx_test_self_attn_multi_kl(_p(q), _p(dk), _p(dv), rows, heads, n_new, N_CTX, d, mq, ch, _p(o), _stream())
            torch.cuda.synchronize()
            assert rc == 0, (mq, ch, rc)
            outs.append(o.cpu().numpy())
        assert np.isfinite(outs[0]).all()
        assert np.array_equal(outs[0], outs[1]), (n_new, mq)


def _guard(shape):
    """f16 NaNs with distinct payloads (0x7c01 .. 0x7fff): a guard value copied to the wrong place is seen, too"""
    n = int(np.prod(shape))
    return torch.from_numpy((0x7c01 + np.arange(n, dtype=np.int64) % 0x3ff).astype(np.int16).reshape(shape)).view(torch.float16)


def test_kv_append_writer_chunked_equals_row_major():
    # the general call with skip_append = 0: kv_append_kernel copies k | v of the new tokens into the cache, then the kernels read them
    lib = _lib()
    rng = np.random.default_rng(5)
    n_new = 9
    pos0 = torch.from_numpy(np.asarray([0, 3, 100, 439, 17, 64, 127], np.int32))
    qkv = torch.from_numpy(rng.standard_normal((R * n_new, 3 * D)).astype(np.float16)).cuda()
    caches = []
    for _ in range(2):                               # older positions hold numbers, the rest the guard
        c = rng.standard_normal((R, N_CTX, D)).astype(np.float16)
        for r in range(R):
            c[r, int(pos0[r]):] = np.float16(np.nan)
        caches.append(torch.from_numpy(c))
    kc_rm, vc_rm = caches
    res = []
    for ch in (0, 1):
        dk = (kc_rm if ch == 0 else _chunked(lib, kc_rm, N_CTX, D)).cuda()
        dv = vc_rm.cuda()
        o = torch.full((R * n_new, D), float("nan"), dtype=torch.half, device="cuda")
        rc = lib.swx_test_self_attn_general_kl(1, _p(qkv), 3 * D, _p(dk), _p(dv), None, _p(pos0.cuda()), R, H, n_new, N_CTX, D, 1, 0, 0, 0, ch,
                                               _p(o), _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        res.append((dk.cpu(), dv.cpu(), o.cpu().numpy()))
    (k0, v0, o0), (k1, v1, o1) = res
    assert np.isfinite(o0).all() and np.array_equal(o0, o1)
    assert np.array_equal(_bits(v0), _bits(v1))
    assert np.array_equal(_bits(_chunked(lib, k0, N_CTX, D)), _bits(k1))
    for r in range(R):
        p = int(pos0[r])
        assert np.array_equal(_bits(k0[r, p:p + n_new]), _bits(qkv[r * n_new:(r + 1) * n_new, D:2 * D]))
        assert torch.isnan(k0[r, p + n_new:]).all() and np.array_equal(_bits(k0[r, :p]), _bits(kc_rm[r, :p]))


# (M, epilogue bits beyond LN | QKV, rows per sequence, debug flags, kernel): bit 6 = a multi-token pass
SCATTER_FORMS = {
    "one_token_per_row": (7, 0, 0, FLAG_DEC_NO_W1, DEC_W4),
    "seven_per_sequence": (21, 64, 7, FLAG_DEC_NO_W1, DEC_W4),
    "tall": (168, 64, 7, 0, DEC_TALL4),
    "single_wave": (5, 0, 0, 0, DEC_W1),
}


@pytest.mark.parametrize("form", list(SCATTER_FORMS))
def test_qkv_scatter_writers_chunked_equals_row_major(form):
    lib = _lib()
    M, extra, rps, flags, kid = SCATTER_FORMS[form]
    d, n_ctx, epi = D, N_CTX, 1 | 8 | extra
    N, K = 3 * d, d
    rng = np.random.default_rng(M)
    n_seq = M // rps if rps else M
    per = rps or 1
    pos0 = rng.integers(0, n_ctx - per + 1, n_seq).astype(np.int32)
    pos0[0], pos0[-1] = 0, n_ctx - per               # both ends of the context
    a = torch.from_numpy(rng.standard_normal((M, K)).astype(np.float16)).cuda()
    w = torch.from_numpy((rng.standard_normal((N, K)) * 0.03).astype(np.float16)).cuda()
    gamma = torch.from_numpy((1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)).cuda()
    beta = torch.from_numpy((0.05 * rng.standard_normal(K)).astype(np.float32)).cuda()
    bias = torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)).cuda()
    tp = torch.from_numpy(pos0).cuda()
    scratch_bytes = N * K * 2 + 8 * N + 16 * M * N * 4 + 8192 + 4096 * 4
    kg, vg = _guard((n_seq, n_ctx, d)), _guard((n_seq, n_ctx, d)).flip(1).contiguous()
    old = lib.swx_debug_flags(-1)
    base = old & ~FLAG_DEC_NO_W1
    res = []
    try:
        lib.swx_debug_flags(base | flags)
        assert lib.swx_test_dec_plan(M, N, K, epi, base | flags) == kid
        for ch in (0, 1):
            kc = (kg if ch == 0 else _chunked(lib, kg, n_ctx, d)).cuda()
            vc = vg.cuda()
            c = torch.zeros(M, d, dtype=torch.float16, device="cuda")
            scratch = torch.zeros(scratch_bytes, dtype=torch.uint8, device="cuda")
            args = (_p(a), K, _p(w), _p(gamma), _p(beta), _p(bias), _p(c), d, None, _p(kc), _p(vc), _p(tp), n_ctx, d, M, N, K, epi)
            if ch == 0:                              # the entry point the existing tests use: it hands in the row-major descriptor
                rc = lib.swx_test_dec_gemm(*args, _p(scratch), scratch.numel(), _stream())
            else:
                rc = lib.swx_test_dec_gemm_kl(*args, rps, 1, _p(scratch), scratch.numel(), _stream())
            torch.cuda.synchronize()
            assert rc == 0, (form, ch, rc)
            res.append((kc.cpu(), vc.cpu(), c.cpu()))
    finally:
        lib.swx_debug_flags(old)
    (k0, v0, c0), (k1, v1, c1) = res
    assert np.array_equal(_bits(c0), _bits(c1)) and np.array_equal(_bits(v0), _bits(v1))
    assert np.array_equal(_bits(_chunked(lib, k0, n_ctx, d)), _bits(k1))
    # the row-major side, stated on its own: exactly the positions of the map are written (finite numbers), the rest is the guard
    written = np.zeros((n_seq, n_ctx), bool)
    for m in range(M):
        written[m // per, pos0[m // per] + m % per] = True
    assert written.sum() == M
    for cache, guard in ((k0, kg), (v0, vg)):
        assert torch.isfinite(cache[torch.from_numpy(written)]).all()
        assert np.array_equal(_bits(cache)[~written], _bits(guard)[~written])
    assert torch.isfinite(c0).all() and float(c0.float().abs().max()) > 0


def test_transcribe_is_equal_with_either_layout():
    import importlib.util
    import os
    import stable_ts_amd as sw
    lib = _lib()
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    audio = mod.synth_audio(75.0, 9)
    dims = sw.dims_for("tiny.en")
    model = sw.Whisper(dims, dtype="f16", max_windows=3, max_rows=15)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
    old = lib.swx_debug_flags(-1)
    out = []
    try:
        for flags in (old | FLAG_CHUNKED, old & ~FLAG_CHUNKED):
            lib.swx_debug_flags(flags)
            res = model.transcribe(audio, language="en", regroup=False, batch_size=3, beam_size=5, word_timestamps=True, sample_len=40,
                                   min_tokens=40, temperature=0.0)
            out.append(json.dumps(res.to_dict(), sort_keys=True))
    finally:
        lib.swx_debug_flags(old)
    assert len(json.loads(out[0])["segments"]) > 0 and any(s["words"] for s in json.loads(out[0])["segments"])
    assert out[0] == out[1]
