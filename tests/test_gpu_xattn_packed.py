"""The decode cross-attention kernels production launches -- attn_decode_cross2_f16<true, 1 | 2 | 4> on the fragment-ordered copy and
attn_decode_cross_xq2_f16<FQ> with the query projection inside -- against float64 attention (scale 0.125) on the f16 values as stored,
through swx_test_attention_packed.  Tolerance: the 6e-3 test_attention_decode_cross_kernel holds this kernel body to (f16 rounding of
the probabilities).  Every launch is first PROVED to be the kernel form it is meant to be (swx_test_xattn_plan: family, QG, depth).
The fragment-ordered copy the kernels read is built on the host by tests/xkv_layout_ref.py, which shares no code with them; in the
chain test it is written by the K | V projection's epilogue instead.  The output buffer carries NaN guard rows that must survive.

Key counts: 128 = one block per wave, no loop; 129 = a last block with one valid key; 132 / 156 = 4 / 28 keys into the last block;
224 / 256 / 288 = 7 / 8 / 9 blocks: an odd and an even number of blocks per wave, the two-block loop ending with and without its
remainder step; 1500 = production.
"""
import ctypes

import numpy as np
import pytest
import torch

import xkv_layout_ref as xr

pytestmark = pytest.mark.gpu

NO_PACKED_XKV, XATTN_R5, XQ_FULL_TILE = 2048, 33554432, 512
NOT_DECODE, ROW, PACKED, PACKED_FQ = 0, 1, 2, 3
GUARD = 3
NAN = float("nan")
TOL = 6e-3


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _plan(family, qg, depth):
    return family + 16 * qg + 256 * depth


class _Flags:
    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.prev = _lib().swx_debug_flags(-1)
        _lib().swx_debug_flags(self.flags)

    def __exit__(self, *exc):
        _lib().swx_debug_flags(self.prev)


def _vt_kp(nk):
    return 1536 if nk > 288 else 320


class _Chunks:
    """K / V [B][nk][d] f16 as the production chunk of every batch item: [ K rows | V^T per head, keys zero padded | fragment-ordered copy ]"""

    def __init__(self, K, V):
        self.B, self.nk, self.d = K.shape
        self.H = self.d // 64
        self.vt_kp = _vt_kp(self.nk)
        self.v_off = self.nk * self.d
        self.p_off = self.v_off + self.d * self.vt_kp
        self.chunk = self.p_off + self.H * xr.per_head(self.nk) + 8
        host = np.zeros((self.B, self.chunk), np.float16)
        for b in range(self.B):
            host[b, :self.v_off] = K[b].ravel()
            vt = np.zeros((self.d, self.vt_kp), np.float16)
            vt[:, :self.nk] = V[b].T
            host[b, self.v_off:self.p_off] = vt.ravel()
            host[b, self.p_off:self.chunk - 8] = xr.packed_from(K[b], V[b], self.nk).ravel()
        self.buf = torch.from_numpy(host).cuda()


def _launch(ck, nq, *, q=None, fq=None, flags=0, want=None, packed=True):
    """one launch on the chunks `ck`; returns the whole output buffer [B * nq + GUARD][d] (CPU f16).  want = (family, QG, depth)"""
    lib = _lib()
    B, H, d = ck.B, ck.H, ck.d
    plan = lib.swx_test_xattn_plan(B, H, nq, ck.nk, ck.vt_kp, 1 if packed else 0, 0 if fq is None else 1, 0, flags)
    assert plan == _plan(*want), (plan, want)
    o = torch.full((B * nq + GUARD, d), NAN, dtype=torch.float16, device="cuda")
    with _Flags(flags):
        if fq is None:
            assert q.shape == (B * nq, d) and q.is_contiguous()
            rc = lib.swx_test_attention_packed(_p(q), d, _p(ck.buf), _p(ck.buf, ck.v_off), d, ck.chunk, ck.chunk,
                                               _p(ck.buf, ck.p_off) if packed else None, _p(o), d, B, H, nq, ck.nk, ck.vt_kp, 0,
                                               None, 0, 0, None, None, None, None, None, 0, _stream())
        else:
            x, wq, gamma, beta, bias, scratch = fq
            rc = lib.swx_test_attention_packed(None, 0, _p(ck.buf), _p(ck.buf, ck.v_off), d, ck.chunk, ck.chunk, _p(ck.buf, ck.p_off),
                                               _p(o), d, B, H, nq, ck.nk, ck.vt_kp, 0, _p(x), d, x.shape[0], _p(wq), _p(gamma), _p(beta),
                                               _p(bias), _p(scratch), scratch.numel(), _stream())
        torch.cuda.synchronize()
    assert rc == 0, rc
    return o.cpu()


def _ref(q, K, V):
    """q [B][nq][d], K / V [B][nk][d] (numpy f16) -> float64 [B * nq][d]"""
    return np.concatenate([xr.attention_f64(q[b], K[b], V[b]) for b in range(q.shape[0])])


def _check(o, ref, what):
    n = ref.shape[0]
    assert torch.isnan(o[n:]).all(), f"{what}: guard rows behind row {n} were written"
    got = o[:n].double().numpy()
    assert not np.isnan(got).any(), f"{what}: rows {np.flatnonzero(np.isnan(got).any(1))[:8]} not written"
    err = np.abs(got - ref)
    r, c = np.unravel_index(int(np.argmax(err)), err.shape)
    print(f"{what}: max error {err.max():.3g} at row {r} column {c} (head {c // 64} dim {c % 64})")
    assert err.max() < TOL, f"{what}: max error {err.max():.3g} at row {r} column {c} (head {c // 64} dim {c % 64})"


def _bits_equal(a, b, what):
    a, b = a.view(torch.int16), b.view(torch.int16)
    if not torch.equal(a, b):
        r, c = (a != b).nonzero()[0].tolist()
        raise AssertionError(f"{what}: bits differ in {int((a != b).sum())} elements, first at row {r} column {c} (head {c // 64} dim {c % 64})")


def _case(B, H, nq, nk, seed):
    rng = np.random.default_rng(seed)
    d = 64 * H
    q = (rng.standard_normal((B, nq, d)) * 1.5).astype(np.float16)      # scores of standard deviation ~1.5: neither flat nor one-hot
    K = rng.standard_normal((B, nk, d)).astype(np.float16)
    V = (rng.standard_normal((B, nk, d)) + 0.25 * np.arange(d) / d).astype(np.float16)
    return q, K, V


@pytest.mark.parametrize("nk", [128, 129, 132, 156, 224, 256, 288, 1500])
@pytest.mark.parametrize("B,H,nq", [(1, 1, 1), (3, 4, 5), (2, 2, 16), (1, 3, 7)])
def test_packed_decode_step(B, H, nq, nk):
    q, K, V = _case(B, H, nq, nk, 1000 * B + 10 * nq + nk)
    ref = _ref(q, K, V)
    ck = _Chunks(K, V)
    qd = torch.from_numpy(q).cuda().view(B * nq, 64 * H)
    two = _launch(ck, nq, q=qd, flags=0, want=(PACKED, 1, 2))
    _check(two, ref, "attn_decode_cross2_f16<true, 1>")
    one = _launch(ck, nq, q=qd, flags=XATTN_R5, want=(PACKED, 1, 1))
    _check(one, ref, "attn_decode_cross_f16<true, 1>")
    row = _launch(ck, nq, q=qd, flags=NO_PACKED_XKV, want=(ROW, 1, 1))
    _check(row, ref, "attn_decode_cross_f16<false, 1>")
    _bits_equal(two, row, "packed, two blocks in flight vs row layout")
    _bits_equal(one, row, "packed, one block in flight vs row layout")


@pytest.mark.parametrize("B,H,nq,nk,qg", [(1, 2, 40, 132, 1), (8, 20, 64, 132, 2), (8, 20, 200, 132, 4), (1, 2, 40, 1500, 1)])
def test_packed_groups_of_16_rows(B, H, nq, nk, qg):
    # 200 rows = 13 groups: the last workgroup of a (window, head) carries ONE group and leaves the merge loop at its `break`
    d = 64 * H
    q, K, V = _case(B, H, nq, nk, B + nq + nk)
    ref = _ref(q, K, V)
    ck = _Chunks(K, V)
    qd = torch.from_numpy(q).cuda()
    whole = _launch(ck, nq, q=qd.view(B * nq, d), want=(PACKED, qg, 2))
    _check(whole, ref, f"attn_decode_cross2_f16<true, {qg}>")
    _check(_launch(ck, nq, q=qd.view(B * nq, d), flags=XATTN_R5, want=(PACKED, qg, 1)), ref, f"attn_decode_cross_f16<true, {qg}>")
    whole = whole[:B * nq].view(B, nq, d)

    def rows(lo, hi, want_qg):
        part = _launch(ck, hi - lo, q=qd[:, lo:hi].contiguous().view(B * (hi - lo), d), want=(PACKED, want_qg, 2))
        assert torch.isnan(part[B * (hi - lo):]).all()
        _bits_equal(part[:B * (hi - lo)].view(B, hi - lo, d), whole[:, lo:hi].contiguous(), f"rows {lo}..{hi} as QG = {want_qg} vs QG = {qg}")

    # QG must not change a bit: every group of 16 rows as a launch of its own (the decode-step form) ...
    for lo in range(0, nq, 16):
        rows(lo, min(lo + 16, nq), 1)
    # ... and the same rows on the other group counts
    if (B, H) == (8, 20):
        for lo in range(0, nq - 63, 64):
            rows(lo, lo + 64, 2)                       # 4 groups: 640 workgroups of one group -> QG = 2
        if nq == 64:
            q4 = torch.cat([qd, qd, qd, qd[:, :8]], 1).contiguous()     # the 64 rows again as rows of a 200-row pass -> QG = 4
            part = _launch(ck, 200, q=q4.view(B * 200, d), want=(PACKED, 4, 2))[:B * 200].view(B, 200, d)
            for lo in (0, 64, 128):
                _bits_equal(part[:, lo:lo + 64].contiguous(), whole.contiguous(), f"rows as QG = 4 at {lo} vs QG = 2")


def _dec_scratch_bytes(M, N, K):
    return N * K * 2 + 8 * N + 16 * M * N * 4 + 8192 + 4096 * 4


# every instantiation FQ = d / 32 at 132 keys; the production key count at the smallest and the largest d only (seconds, not minutes)
_FQ_CASES = [(d, nq, B, nk) for nk in (132, 1500) for d in (384, 512, 640, 768, 1024, 1280) for nq in (1, 5, 16) for B in (1, 3)
             if nk == 132 or d in (384, 1280)]


@pytest.mark.parametrize("d,nq,B,nk", _FQ_CASES)
def test_fused_query_projection(d, nq, B, nk):
    lib = _lib()
    H, M = d // 64, B * nq
    rng = np.random.default_rng(d + 100 * nq + B + nk)
    # residual rows with a per-row scale 0.5 .. 4 and offset +-2 (the inputs of test_dec_gemm_layernorm_fold): the statistics matter.
    # Wq ~ N(0, 1 / d): LN(x) has unit variance per element, so q has variance ~1 -- scores of standard deviation ~1 after the 1 / 8
    x = (rng.standard_normal((M, d)) * rng.uniform(0.5, 4.0, (M, 1)) + rng.uniform(-2, 2, (M, 1))).astype(np.float16)
    wq = (rng.standard_normal((d, d)) / np.sqrt(d)).astype(np.float16)
    gamma = (1.0 + 0.2 * rng.standard_normal(d)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(d)).astype(np.float32)
    bias = (0.1 * rng.standard_normal(d)).astype(np.float32)
    K = rng.standard_normal((B, nk, d)).astype(np.float16)
    V = (rng.standard_normal((B, nk, d)) + 0.25 * np.arange(d) / d).astype(np.float16)
    ck = _Chunks(K, V)
    xd, wd, gd, bd, biasd = (torch.from_numpy(t).cuda() for t in (x, wq, gamma, beta, bias))

    # q of the separate launch: the decode-step GEMM with its LayerNorm epilogue on the same x / Wq
    qd = torch.full((M + GUARD, d), NAN, dtype=torch.float16, device="cuda")
    scratch = torch.empty(_dec_scratch_bytes(M, d, d), dtype=torch.uint8, device="cuda")
    rc = lib.swx_test_dec_gemm(_p(xd), d, _p(wd), _p(gd), _p(bd), _p(biasd), _p(qd), d, None, None, None, None, 0, 0, M, d, d, 1,
                               _p(scratch), scratch.numel(), _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    q = qd[:M].cpu().numpy()
    assert np.isfinite(q).all() and 0.5 < q.astype(np.float64).std() < 2.0, q.astype(np.float64).std()
    unfused = _launch(ck, nq, q=qd[:M], want=(PACKED, 1, 2))
    # (b) float64 attention on the q as stored and the K / V as stored
    ref = _ref(q.reshape(B, nq, d), K, V)
    _check(unfused, ref, "unfused, q from the decode-step GEMM")
    # (a) the projection inside the launch: the same bits, staging the window's rows only and the whole 16-row tile
    fq = (xd, wd, gd, bd, biasd, torch.empty(d * d * 2 + 8 * d + 1024, dtype=torch.uint8, device="cuda"))
    for flags, depth in ((0, 2), (XQ_FULL_TILE, 2), (XATTN_R5, 1)):
        fused = _launch(ck, nq, fq=fq, flags=flags, want=(PACKED_FQ, 1, depth))
        _check(fused, ref, f"attn_decode_cross_xq{'2' if depth == 2 else ''}_f16<{d // 32}> flags {flags}")
        _bits_equal(fused, unfused, f"fused query projection (flags {flags}) vs the separate launch")


def test_plan_families():
    lib = _lib()
    plan = lib.swx_test_xattn_plan
    assert plan(2, 6, 5, 1500, 1536, 0, 0, 0, 0) == _plan(ROW, 1, 1)            # no copy: the row layout
    assert plan(2, 6, 5, 1500, 1536, 1, 0, 0, NO_PACKED_XKV) == _plan(ROW, 1, 1)
    assert plan(2, 6, 5, 1500, 1536, 1, 0, 3, 0) == _plan(PACKED, 1, 2)
    assert plan(2, 6, 5, 100, 1536, 1, 0, 0, 0) == _plan(NOT_DECODE, 1, 1)      # fewer than 128 keys
    assert plan(2, 6, 5, 100, 1536, 1, 0, 3, 0) < 0
    assert plan(2, 6, 40, 1500, 1536, 0, 0, 0, 0) == _plan(NOT_DECODE, 1, 1)    # groups of rows need the copy
    assert plan(2, 6, 5, 1500, 0, 1, 0, 0, 0) == _plan(NOT_DECODE, 1, 1)        # row-major V
    assert plan(2, 6, 5, 1500, 1536, 1, 1, 0, 0) == _plan(PACKED_FQ, 1, 2)
    assert plan(2, 6, 5, 1500, 1536, 0, 1, 0, 0) < 0                            # the fused query reads the copy only
    assert plan(2, 6, 40, 1500, 1536, 1, 1, 0, 0) < 0                           # ... and one group of rows
    assert plan(2, 7, 5, 1500, 1536, 1, 1, 0, 0) < 0                            # d = 448: no instantiation


@pytest.mark.parametrize("S,B,nq", [(132, 3, 5), (156, 3, 16), (1500, 2, 5)])
def test_chain_projection_epilogue_to_attention(S, B, nq):
    """xa -> K | V projection whose epilogue writes the row layout AND the fragment-ordered copy -> attention on the copy.  Reference:
    float64 attention on the K / V the projection stored, read back from the ROW layout by tests/xkv_layout_ref.py's index functions: the
    producer, the layout statement and the consumer have to agree without sharing code."""
    lib = _lib()
    d, H, Kd = 128, 2, 128
    vt_kp = _vt_kp(S)
    g = torch.Generator().manual_seed(S + B)
    xa = (torch.randn(B * S, Kd, generator=g) * (0.5 + torch.rand(B * S, 1, generator=g))).half().cuda()
    w = (torch.randn(2 * d, Kd, generator=g) / Kd ** 0.5).half().cuda()
    bias = torch.randn(2 * d, generator=g).cuda()
    q = (torch.randn(B * nq, d, generator=g) * 1.5).half().cuda()
    v_off = S * d
    p_off = v_off + d * vt_kp
    chunk = p_off + H * xr.per_head(S) + 8
    buf = torch.full((B, chunk), NAN, dtype=torch.float16, device="cuda")
    # V^T's own key padding is the caller's in production (swx_pad_zero); here too
    for b in range(B):
        buf[b, v_off:p_off].view(d, vt_kp)[:, S:] = 0
    rc = lib.swx_test_gemm_layout(1, _p(xa), Kd, _p(w), Kd, _p(bias), None, None, 0, _p(buf), d, _p(buf, v_off), _p(buf, p_off), chunk,
                                  xr.ceil32(S), d, S, vt_kp, chunk, 0, B * S, 2 * d, Kd, 1 | 128, 0, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    flat = host.ravel()
    key, col = np.meshgrid(np.arange(S), np.arange(d), indexing="ij")
    Ks = np.stack([flat[xr.cbatch_index(b * S + key, col, S, chunk, d)] for b in range(B)])
    Vs = np.stack([flat[v_off + xr.vt_index(b, col // 64, col % 64, key, vt_kp, chunk)] for b in range(B)])
    assert np.isfinite(Ks).all() and np.isfinite(Vs).all()
    ref = _ref(q.cpu().numpy().reshape(B, nq, d), Ks, Vs)
    plan = lib.swx_test_xattn_plan(B, H, nq, S, vt_kp, 1, 0, 0, lib.swx_debug_flags(-1))
    assert plan == _plan(PACKED, 1, 2), plan
    o = torch.full((B * nq + GUARD, d), NAN, dtype=torch.float16, device="cuda")
    # the row-layout pointers are withheld: the launch can read the copy only
    rc = lib.swx_test_attention_packed(_p(q), d, None, None, 0, chunk, chunk, _p(buf, p_off), _p(o), d, B, H, nq, S, vt_kp, 0,
                                       None, 0, 0, None, None, None, None, None, 0, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _check(o.cpu(), ref, f"chain S = {S}")
