"""The layout epilogues of the GEMM kernels and the stand-alone packer against float64, in isolation (swx_test_gemm_layout,
swx_test_xkv_pack), at the smallest shapes where they can go wrong: three batch items of 128 / 132 / 156 rows (a 128-row tile
straddles two items, the last tile is partial, a batch item ends 0 / 4 / 28 keys into a 32-key block), on every kernel the plan
offers for the epilogue.

Every destination is filled with NaN first and compared WHOLE: an element the reference writes is within tolerance, every other
element is still NaN -- or an exact zero where the epilogue owns the padding.  Where a value lives is stated by
tests/xkv_layout_ref.py (index arithmetic of its own; the fragment-ordered copy from the consumer's MFMA operand meaning).
Tolerances: f16 2e-3 max|ref| + 1e-3 (one rounding of the output, test_gemm_f16_tiled_and_skinny), f32 3e-6 sum|a||w| + 1e-6
(test_gemm_f32_exact_mode), GELU cases 4e-3 / 1e-5 max(1, max|gelu|) (test_gemm_epilogues).
"""
import ctypes

import numpy as np
import pytest
import torch

import xkv_layout_ref as xr

pytestmark = pytest.mark.gpu

BIAS, GELU, OUT_F32, RESF32MOD, STORE_VT, CBATCH, KV, QKV_VT = 1, 2, 8, 16, 32, 64, 128, 256
TILED_REG, SKINNY, GLDS128, GLDS64, RING64, RING128 = 0, 1, 2, 3, 4, 5
B = 3
NAN = float("nan")


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _p(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + off * t.element_size())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cdiv(a, b):
    return (a + b - 1) // b


def _kernels(M, N, K, epi):
    """[(force_kernel, kernel id)] of every forced tiled f16 kernel, each PROVED through the plan to be the kernel it is meant to be"""
    lib = _lib()
    flags = lib.swx_debug_flags(-1)
    narrow = N % 64 == 0 and _cdiv(N, 128) * _cdiv(M, 128) < 224
    want = {1: TILED_REG, 7: GLDS64 if narrow else GLDS128, 8: GLDS64, 9: GLDS128, 10: RING64, 11: RING128}
    out = []
    for force, kid in want.items():
        plan = lib.swx_test_gemm_plan(M, N, K, epi, force, flags)
        if K % 64 != 0 and force >= 7:
            assert plan < 0, (force, plan)          # direct-to-LDS kernels need whole 64-deep K steps: refused, not skipped
            continue
        assert plan == kid, (force, plan, kid)
        out.append((force, kid))
    return out


def _width(kid):
    return 64 if kid in (GLDS64, RING64) else 128


def _call(dtype, a, lda, w, *, M, N, K, epi, c, ldc, bias=None, resf=None, res_mod=0, c2_off=None, p_off=None, p_bs=0, p_nkpad=0,
          p_vcol0=0, vt_s=0, vt_kp=0, vt_bs=0, zero_pad=0, force=0, ldw=None):
    lib = _lib()
    rc = lib.swx_test_gemm_layout(dtype, _p(a), lda, _p(w), ldw or w.stride(0), _p(bias), None, _p(resf), res_mod, _p(c), ldc,
                                  None if c2_off is None else _p(c, c2_off), None if p_off is None else _p(c, p_off), p_bs, p_nkpad,
                                  p_vcol0, vt_s, vt_kp, vt_bs, zero_pad, M, N, K, epi, force, _stream())
    torch.cuda.synchronize()
    return rc


def _inputs(M, N, K, seed, tdt=torch.float16):
    g = torch.Generator().manual_seed(seed)
    a = (torch.randn(M, K, generator=g) * 0.5 * (0.5 + torch.rand(M, 1, generator=g))).to(tdt)
    w = (torch.randn(N, K, generator=g) * 0.5).to(tdt)
    bias = torch.randn(N, generator=g)
    return a, w, bias


def _lin(a, w, bias):
    return (a.double() @ w.double().T + bias.double()).numpy()


def _check_whole(got, expect, tol, zero=None, what=""):
    """got: the whole destination (float64 copy); expect: the same shape, NaN where nothing may be written; zero: mask of elements that must be
    exact zeros.  tol: a scalar or an array of expect's shape."""
    got, expect = np.asarray(got, np.float64).ravel(), np.asarray(expect, np.float64).ravel()
    written = ~np.isnan(expect)
    if zero is not None:
        zero = np.asarray(zero).ravel()
        assert not (zero & written).any()
        bad = np.flatnonzero(zero & ~((got == 0) & ~np.signbit(got)))
        assert bad.size == 0, f"{what}: {bad.size} padding elements are not +0, first at flat index {bad[0]} = {got[bad[0]]}"
        untouched = ~written & ~zero
    else:
        untouched = ~written
    bad = np.flatnonzero(untouched & ~np.isnan(got))
    assert bad.size == 0, f"{what}: {bad.size} elements written outside the layout, first at flat index {bad[0]} = {got[bad[0]]}"
    bad = np.flatnonzero(written & np.isnan(got))
    assert bad.size == 0, f"{what}: {bad.size} elements of the layout not written, first at flat index {bad[0]}"
    err = np.where(written, np.abs(got - np.where(written, expect, 0.0)), 0.0)
    over = err > (tol if np.isscalar(tol) else np.asarray(tol, np.float64).ravel())
    i = int(np.argmax(err))
    print(f"{what}: max error {err.max():.3g} at flat index {i} (got {got[i]:.6g}, reference {expect[i]:.6g})")
    assert not over.any(), f"{what}: {int(over.sum())} elements out of tolerance, first at flat index {int(np.flatnonzero(over)[0])}, max error {err.max():.3g}"


def _tol16(ref):
    return 2e-3 * float(np.abs(ref).max()) + 1e-3


def _scatter_cbatch(expect, ref, vt_s, vt_bs, ldc, base=0):
    M, N = ref.shape
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    expect[base + xr.cbatch_index(m, n, vt_s, vt_bs, ldc)] = ref


def _scatter_vt(expect, ref, vt_s, vt_kp, vt_bs, base=0):
    M, N = ref.shape
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    expect[base + xr.vt_index(m // vt_s, n // 64, n % 64, m % vt_s, vt_kp, vt_bs)] = ref


def _pad_mask(size, nb, N, vt_s, vt_kp, vt_bs, base=0):
    zero = np.zeros(size, bool)
    b, n, key = np.meshgrid(np.arange(nb), np.arange(N), np.arange(vt_s, vt_kp), indexing="ij")
    zero[base + xr.vt_index(b, n // 64, n % 64, key, vt_kp, vt_bs)] = True
    return zero


# (d, K, vt_s, vt_kp): d and K in {128, 384}, vt_s in {128, 132, 156} (M = 384 / 396 / 468), vt_kp in {160, 1536}, each value at least twice
COMBOS = [(128, 128, 128, 160), (128, 384, 132, 160), (384, 128, 156, 160), (384, 384, 132, 1536), (128, 128, 156, 1536),
          (384, 384, 128, 160)]


@pytest.mark.parametrize("d,K,vt_s,vt_kp", COMBOS)
def test_cbatch_and_store_vt_alone(d, K, vt_s, vt_kp):
    M, N = B * vt_s, d
    a, w, bias = _inputs(M, N, K, d + K + vt_s)
    ref = _lin(a, w, bias)
    a, w, bias = a.cuda(), w.cuda(), bias.cuda()
    tol = _tol16(ref)
    for force, kid in _kernels(M, N, K, BIAS | CBATCH):
        # rows grouped per batch item: a row pitch with 8 spare columns and 40 spare elements between the items, all of which stay NaN
        ldc, vt_bs = N + 8, vt_s * (N + 8) + 40
        c = torch.full((B * vt_bs + 16,), NAN, dtype=torch.float16, device="cuda")
        assert _call(1, a, K, w, M=M, N=N, K=K, epi=BIAS | CBATCH, c=c, ldc=ldc, bias=bias, vt_s=vt_s, vt_bs=vt_bs, force=force) == 0
        expect = np.full(c.numel(), NAN)
        _scatter_cbatch(expect, ref, vt_s, vt_bs, ldc)
        _check_whole(c.cpu().double().numpy(), expect, tol, what=f"CBATCH kernel {kid}")
        # transposed per head, keys contiguous; the key padding [vt_s, vt_kp) is NOT this epilogue's: it stays NaN
        vt_bs = N * vt_kp + 32
        c = torch.full((B * vt_bs + 16,), NAN, dtype=torch.float16, device="cuda")
        assert _call(1, a, K, w, M=M, N=N, K=K, epi=BIAS | STORE_VT, c=c, ldc=N, bias=bias, vt_s=vt_s, vt_kp=vt_kp, vt_bs=vt_bs,
                     force=force) == 0
        expect = np.full(c.numel(), NAN)
        _scatter_vt(expect, ref, vt_s, vt_kp, vt_bs)
        _check_whole(c.cpu().double().numpy(), expect, tol, what=f"STORE_VT kernel {kid}")


def _kv_case(d, K, vt_s, vt_kp, with_p, forces=None, nb=B):
    """EPI_KV over the production chunk of a batch item: [ K rows vt_s x d | V^T d x vt_kp | fragment-ordered copy | 16 spare ]"""
    M, N, H = nb * vt_s, 2 * d, d // 64
    a, w, bias = _inputs(M, N, K, 3 * d + K + vt_s + nb)
    ref = _lin(a, w, bias)
    a, w, bias = a.cuda(), w.cuda(), bias.cuda()
    tol = _tol16(ref)
    per_head = xr.per_head(vt_s)
    v_off = vt_s * d
    p_off = v_off + d * vt_kp
    chunk = p_off + H * per_head + 16
    ran = 0
    for force, kid in _kernels(M, N, K, BIAS | KV):
        if forces is not None and force not in forces:
            continue
        c = torch.full((nb * chunk,), NAN, dtype=torch.float16, device="cuda")
        kw = dict(p_off=p_off, p_bs=chunk, p_nkpad=xr.ceil32(vt_s), p_vcol0=d) if with_p else {}
        rc = _call(1, a, K, w, M=M, N=N, K=K, epi=BIAS | KV, c=c, ldc=d, bias=bias, c2_off=v_off, vt_s=vt_s, vt_kp=vt_kp, vt_bs=chunk,
                   force=force, **kw)
        if d % _width(kid) != 0:
            assert rc == -2, (kid, rc)              # the column split inside a tile: refused by rule, nothing launched
            assert torch.isnan(c).all()
            continue
        assert rc == 0, (kid, rc)
        ran += 1
        got = c.cpu()
        expect = np.full(c.numel(), NAN)
        _scatter_cbatch(expect, ref[:, :d], vt_s, chunk, d)
        _scatter_vt(expect, ref[:, d:], vt_s, vt_kp, chunk, base=v_off)
        g64 = got.double().numpy()
        if with_p:      # the copy is compared below, bit for bit: mask it out of the whole-buffer comparison
            for b in range(nb):
                g64[b * chunk + p_off:b * chunk + p_off + H * per_head] = NAN
        _check_whole(g64, expect, tol, what=f"KV kernel {kid} P={with_p}")
        if with_p:
            gb = got.view(nb, chunk)
            for b in range(nb):
                k_st = gb[b, :v_off].view(vt_s, d).numpy()
                v_st = gb[b, v_off:p_off].view(d, vt_kp)[:, :vt_s].T.contiguous().numpy()
                want = xr.packed_from(k_st, v_st, vt_s)              # the same f16 values, stored twice; padding keys zero
                have = gb[b, p_off:p_off + H * per_head].view(H, per_head).numpy()
                diff = np.flatnonzero(want.view(np.uint16).ravel() != have.view(np.uint16).ravel())
                if diff.size:
                    kind, key, dim = xr.slot_map(vt_s)
                    s = diff[0] % per_head
                    raise AssertionError(f"KV kernel {kid}: packed copy of batch item {b} differs in {diff.size} halfs; first: head "
                                         f"{diff[0] // per_head} slot {s} = {'KV'[kind[s]]} key {key[s]} dim {dim[s]}: "
                                         f"{have.ravel()[diff[0]]} != {want.ravel()[diff[0]]}")
    return ran


@pytest.mark.parametrize("with_p", [False, True])
@pytest.mark.parametrize("d,K,vt_s,vt_kp", COMBOS)
def test_kv_one_launch_with_and_without_the_packed_copy(d, K, vt_s, vt_kp, with_p):
    assert _kv_case(d, K, vt_s, vt_kp, with_p) == 6


@pytest.mark.parametrize("with_p", [False, True])
def test_kv_split_inside_a_128_column_tile_is_refused(with_p):
    # d = 192: the K | V split is a multiple of the 64-column tiles only -- the three 64-column launches run and are checked, the
    # three 128-column ones return an error
    assert _kv_case(192, 128, 132, 160, with_p) == 3


def test_kv_production_length():
    # vt_s = 1500 (28 keys into the last block, as in production), two batch items; on the dispatcher's kernel and the reference kernel
    assert _kv_case(128, 128, 1500, 1536, True, forces=(1, 7, 11), nb=2) == 3


@pytest.mark.parametrize("d,K,vt_s,vt_kp", COMBOS)
def test_qkv_vt_zeroes_the_key_padding(d, K, vt_s, vt_kp):
    M, N = B * vt_s, 3 * d
    a, w, bias = _inputs(M, N, K, 5 * d + K + vt_s)
    ref = _lin(a, w, bias)
    a, w, bias = a.cuda(), w.cuda(), bias.cuda()
    tol = _tol16(ref)
    vt_bs = d * vt_kp + 32
    c2_off = M * N + 8
    for force, kid in _kernels(M, N, K, BIAS | QKV_VT):
        c = torch.full((c2_off + B * vt_bs + 16,), NAN, dtype=torch.float16, device="cuda")
        assert _call(1, a, K, w, M=M, N=N, K=K, epi=BIAS | QKV_VT, c=c, ldc=N, bias=bias, c2_off=c2_off, vt_s=vt_s, vt_kp=vt_kp,
                     vt_bs=vt_bs, zero_pad=1, force=force) == 0
        expect = np.full(c.numel(), NAN)
        q_k = np.full((M, N), NAN)
        q_k[:, :2 * d] = ref[:, :2 * d]                    # Q | K plain; the V columns of C are not written
        expect[:M * N] = q_k.ravel()
        _scatter_vt(expect, ref[:, 2 * d:], vt_s, vt_kp, vt_bs, base=c2_off)
        zero = _pad_mask(c.numel(), B, d, vt_s, vt_kp, vt_bs, base=c2_off)
        _check_whole(c.cpu().double().numpy(), expect, tol, zero=zero, what=f"QKV_VT kernel {kid}")


def _gelu64(x):
    return torch.nn.functional.gelu(torch.from_numpy(x)).numpy()


@pytest.mark.parametrize("dtype", [1, 0])
@pytest.mark.parametrize("d,vt_s", [(128, 132), (384, 156)])
def test_conv2_form_overlapping_rows_and_row_modulo_residual(dtype, d, vt_s):
    # out[m] = gelu(A[m] W^T + b) + Rf[m % res_mod] with A[m] = buf[2 d m .. 2 d m + 3 d): lda = 2 d < K = 3 d
    M, N, K = B * vt_s, d, 3 * d
    tdt = torch.float16 if dtype else torch.float32
    g = torch.Generator().manual_seed(d + vt_s)
    buf = (torch.randn((2 * M + 1) * d, generator=g) * 0.5).to(tdt)
    w = (torch.randn(N, K, generator=g) * 0.1).to(tdt)
    bias = torch.randn(N, generator=g)
    rf = torch.randn(vt_s, N, generator=g)
    a_eff = buf.as_strided((M, K), (2 * d, 1))
    gelu = _gelu64(_lin(a_eff, w, bias))
    ref = gelu + rf.double().numpy()[np.arange(M) % vt_s]
    tol = (4e-3 if dtype else 1e-5) * max(1.0, float(np.abs(gelu).max()))
    a_dev = torch.cat([buf, torch.full((4 * d,), NAN, dtype=tdt)]).cuda()      # NaN behind the last row: an over-read shows up
    w, bias, rf = w.cuda(), bias.cuda(), rf.cuda()
    epi = BIAS | GELU | RESF32MOD
    for force, kid in (_kernels(M, N, K, epi) if dtype else [(0, "f32 128x128")]):
        c = torch.full((M + 4, N), NAN, dtype=tdt, device="cuda")
        assert _call(dtype, a_dev, 2 * d, w, M=M, N=N, K=K, epi=epi, c=c, ldc=N, bias=bias, resf=rf, res_mod=vt_s, force=force) == 0
        expect = np.full((M + 4, N), NAN)
        expect[:M] = ref
        _check_whole(c.cpu().double().numpy(), expect, tol, what=f"conv2 form dtype {dtype} kernel {kid}")


@pytest.mark.parametrize("Cp,N,M", [(96, 128, 396), (128, 384, 468), (96, 384, 132)])
def test_conv1_form_against_f64_conv1d(Cp, N, M):
    # A row t = x[t .. t + 2][:] of a channel-last signal with M + 2 rows: lda = Cp, K = 3 Cp (288: no whole 64-deep K steps -> the
    # register-staged kernel only).  Reference: float64 conv1d of the same values (weights tap-major: W[n][tap * Cp + c]).
    K = 3 * Cp
    g = torch.Generator().manual_seed(Cp + N + M)
    x = (torch.randn(M + 2, Cp, generator=g) * 0.5).half()
    w = (torch.randn(N, K, generator=g) * 0.1).half()
    bias = torch.randn(N, generator=g)
    conv = torch.nn.functional.conv1d(x.double().T[None], w.double().view(N, 3, Cp).permute(0, 2, 1), bias.double())[0].T.numpy()
    gelu = _gelu64(conv)
    tol = 4e-3 * max(1.0, float(np.abs(gelu).max()))
    a_dev = torch.cat([x, torch.full((8, Cp), NAN, dtype=torch.float16)]).cuda()   # exactly M + 2 rows, then NaN guard rows
    w, bias = w.cuda(), bias.cuda()
    kernels = _kernels(M, N, K, BIAS | GELU)
    assert [k for _, k in kernels] == ([TILED_REG] if K % 64 else [TILED_REG, GLDS64, GLDS64, GLDS128, RING64, RING128])
    if K % 64:
        assert _lib().swx_test_gemm_plan(M, N, K, BIAS | GELU, 0, 0) == TILED_REG
    for force, kid in kernels + [(0, "dispatch")]:
        c = torch.full((M + 4, N), NAN, dtype=torch.float16, device="cuda")
        assert _call(1, a_dev, Cp, w, M=M, N=N, K=K, epi=BIAS | GELU, c=c, ldc=N, bias=bias, force=force) == 0
        expect = np.full((M + 4, N), NAN)
        expect[:M] = gelu
        _check_whole(c.cpu().double().numpy(), expect, tol, what=f"conv1 form Cp {Cp} kernel {kid}")


@pytest.mark.parametrize("case", ["store_vt_kp_not_4", "cbatch_bs_not_8", "cbatch_ldc_not_8", "plain_ldc_not_8"])
def test_slow_branches_of_the_fast_path_conditions(case):
    d, K, vt_s = 128, 128, 132
    M, N = B * vt_s, d
    a, w, bias = _inputs(M, N, K, 11)
    ref = _lin(a, w, bias)
    a, w, bias = a.cuda(), w.cuda(), bias.cuda()
    tol = _tol16(ref)
    epi = BIAS | (STORE_VT if case == "store_vt_kp_not_4" else 0 if case == "plain_ldc_not_8" else CBATCH)
    for force, kid in _kernels(M, N, K, epi):
        if case == "store_vt_kp_not_4":
            vt_kp, vt_bs = 158, N * 158 + 6
            size = B * vt_bs + 16
            kw = dict(ldc=N, vt_s=vt_s, vt_kp=vt_kp, vt_bs=vt_bs)
        elif case == "plain_ldc_not_8":
            ldc = N + 4
            size = M * ldc + 16
            kw = dict(ldc=ldc)
        else:
            ldc = N + (4 if case == "cbatch_ldc_not_8" else 8)
            vt_bs = vt_s * ldc + (8 if case == "cbatch_ldc_not_8" else 4)
            size = B * vt_bs + 16
            kw = dict(ldc=ldc, vt_s=vt_s, vt_bs=vt_bs)
        c = torch.full((size,), NAN, dtype=torch.float16, device="cuda")
        assert _call(1, a, K, w, M=M, N=N, K=K, epi=epi, c=c, bias=bias, force=force, **kw) == 0
        expect = np.full(size, NAN)
        if case == "store_vt_kp_not_4":
            _scatter_vt(expect, ref, vt_s, vt_kp, vt_bs)
        elif case == "plain_ldc_not_8":
            _scatter_cbatch(expect, ref, M, 0, ldc)
        else:
            _scatter_cbatch(expect, ref, vt_s, vt_bs, ldc)
        _check_whole(c.cpu().double().numpy(), expect, tol, what=f"{case} kernel {kid}")


@pytest.mark.parametrize("vt_s,N,force", [(132, 128, 0), (156, 384, 0), (40, 256, 0), (40, 256, 8), (36, 2560, 0), (36, 2560, 8)])
def test_f32_layout_epilogues(vt_s, N, force):
    # strict mode: every epilogue element-wise (epilogue_store<float>).  M = 396 / 468: gemm_f32_tiled<128, 128, 4>; M = 120 / 108 with
    # N >= 256: the few-row kernels -- 64-deep K chunks by default, the 16-deep generation with force 8, 16 / 32 columns per workgroup
    M, K, vt_kp = B * vt_s, 128, 160
    a, w, bias = _inputs(M, N, K, vt_s + N, torch.float32)
    g = torch.Generator().manual_seed(vt_s)
    rf = torch.randn(vt_s, N, generator=g)
    ref = _lin(a, w, bias)
    bound = (a.double().abs() @ w.double().abs().T + bias.double().abs()).numpy()
    a, w, bias, rfd = a.cuda(), w.cuda(), bias.cuda(), rf.cuda()

    ldc, vt_bs = N + 3, vt_s * (N + 3) + 5
    c = torch.full((B * vt_bs + 16,), NAN, dtype=torch.float32, device="cuda")
    assert _call(0, a, K, w, M=M, N=N, K=K, epi=BIAS | CBATCH, c=c, ldc=ldc, bias=bias, vt_s=vt_s, vt_bs=vt_bs, force=force) == 0
    expect, tol = np.full(c.numel(), NAN), np.zeros(c.numel())
    _scatter_cbatch(expect, ref, vt_s, vt_bs, ldc)
    _scatter_cbatch(tol, 3e-6 * bound + 1e-6, vt_s, vt_bs, ldc)
    _check_whole(c.cpu().double().numpy(), expect, tol, what="f32 CBATCH")

    vt_bs = N * vt_kp + 7
    c = torch.full((B * vt_bs + 16,), NAN, dtype=torch.float32, device="cuda")
    assert _call(0, a, K, w, M=M, N=N, K=K, epi=BIAS | STORE_VT, c=c, ldc=N, bias=bias, vt_s=vt_s, vt_kp=vt_kp, vt_bs=vt_bs,
                 force=force) == 0
    expect, tol = np.full(c.numel(), NAN), np.zeros(c.numel())
    _scatter_vt(expect, ref, vt_s, vt_kp, vt_bs)
    _scatter_vt(tol, 3e-6 * bound + 1e-6, vt_s, vt_kp, vt_bs)
    _check_whole(c.cpu().double().numpy(), expect, tol, what="f32 STORE_VT")

    c = torch.full((M + 4, N), NAN, dtype=torch.float32, device="cuda")
    assert _call(0, a, K, w, M=M, N=N, K=K, epi=BIAS | RESF32MOD, c=c, ldc=N, bias=bias, resf=rfd, res_mod=vt_s, force=force) == 0
    rfm = rf.double().numpy()[np.arange(M) % vt_s]
    expect, tol = np.full((M + 4, N), NAN), np.zeros((M + 4, N))
    expect[:M] = ref + rfm
    tol[:M] = 3e-6 * (bound + np.abs(rfm)) + 1e-6
    _check_whole(c.cpu().double().numpy(), expect, tol, what="f32 RESF32MOD")


def test_combinations_no_kernel_implements_are_refused():
    d, K, vt_s, vt_kp = 128, 128, 132, 160
    M = B * vt_s
    a, w, bias = (t.cuda() for t in _inputs(M, 2 * d, K, 1))
    c = torch.full((B * (vt_s * d + d * vt_kp + 8192 + 16),), NAN, dtype=torch.float16, device="cuda")
    base = dict(M=M, N=2 * d, K=K, c=c, ldc=d, bias=bias, c2_off=vt_s * d, vt_s=vt_s, vt_kp=vt_kp, vt_bs=vt_s * d + d * vt_kp + 8208)
    assert _call(1, a, K, w, epi=BIAS | KV | CBATCH, **base) == -2                                  # two layouts at once
    assert _call(1, a, K, w, epi=BIAS | KV, **{**base, "vt_kp": 158}) == -2                        # V half off the 4-row path
    assert _call(1, a, K, w, epi=BIAS | CBATCH, **base, zero_pad=1) == -2                          # padding without QKV_VT
    assert _call(1, a, K, w, epi=BIAS | CBATCH, **base, p_off=vt_s * d + d * vt_kp, p_bs=base["vt_bs"], p_nkpad=160, p_vcol0=d) == -2
    assert _call(0, a.float(), K, w.float(), epi=BIAS | KV, **base) == -2                          # f32 has no fused K | V launch
    assert _call(1, a, K, w, epi=BIAS | KV, **{**base, "M": 100}) == -2                            # skinny kernel
    assert _call(1, a, K, w, epi=BIAS | STORE_VT, **{**base, "vt_s": 0}) == -1
    assert torch.isnan(c).all()


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("nk", [128, 132, 156, 160, 1500])
def test_xkv_pack_kernel(nk, H):
    # the stand-alone packer on random K / V^T: equal bytes to packed_from, zero padding keys, nothing written past H * per_head
    nb, d = 2, 64 * H
    vt_kp = 1536 if nk > 160 else 160
    per_head = xr.per_head(nk)
    rng = np.random.default_rng(nk + H)
    K = rng.standard_normal((nb, nk, d)).astype(np.float16)
    V = rng.standard_normal((nb, nk, d)).astype(np.float16)
    K[K == 0] = 1
    V[V == 0] = 1
    v_off = nk * d
    p_off = v_off + d * vt_kp
    chunk = p_off + H * per_head + 64
    host = np.full((nb, chunk), np.nan, np.float16)
    for b in range(nb):
        host[b, :v_off] = K[b].ravel()
        vt = np.zeros((d, vt_kp), np.float16)                   # keys contiguous, zero padded past nk
        vt[:, :nk] = V[b].T
        host[b, v_off:p_off] = vt.ravel()
    buf = torch.from_numpy(host).cuda()
    rc = _lib().swx_test_xkv_pack(_p(buf), _p(buf, v_off), _p(buf, p_off), nb, H, nk, d, vt_kp, chunk, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :p_off].view(np.uint16), host[:, :p_off].view(np.uint16))        # the sources are not touched
    assert np.isnan(got[:, p_off + H * per_head:]).all()
    kind, key, dim = xr.slot_map(nk)
    for b in range(nb):
        want = xr.packed_from(K[b], V[b], nk)
        have = got[b, p_off:p_off + H * per_head].reshape(H, per_head)
        assert (have[:, key >= nk] == 0).all()
        diff = np.flatnonzero(want.view(np.uint16).ravel() != have.view(np.uint16).ravel())
        if diff.size:
            s = diff[0] % per_head
            raise AssertionError(f"batch item {b}: {diff.size} halfs differ; first: head {diff[0] // per_head} slot {s} = "
                                 f"{'KV'[kind[s]]} key {key[s]} dim {dim[s]}: {have.ravel()[diff[0]]} != {want.ravel()[diff[0]]}")
