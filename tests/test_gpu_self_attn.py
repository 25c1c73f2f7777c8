"""The cached self-attention family of the decoder (csrc/swx_selfattn.hip) against the float64 reference of tests/self_attn_ref.py.

Until this file the family was tested as "bit-identical to self_attn_cached<f16>", and self_attn_cached only end to end.  Here every
kernel -- the general kernel in f16 and f32 with its append, the multi-token kernels, the single-token step kernels with one and
five rows per workgroup -- runs on caches whose unreferenced entries are NaN, at every position where a lane stride or a chunk of
the step kernels begins or ends, and is compared with the reference elementwise:

    |got - ref| <= u |ref| + 2e-5 A + 1e-7,   u = 2^-11 (f16) / 2^-24 (f32),  A = sum_j p_j |v_j|

(the tolerance and what it covers: tests/self_attn_ref.py; conditions on the cases: tests/test_self_attn_ref_cpu.py).  Every case
asserts, through swx_test_self_attn_plan, that the launch takes the kernel the case is named after.
"""
import ctypes

import numpy as np
import pytest
import torch

import self_attn_ref as sr

pytestmark = pytest.mark.gpu


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _case_and_reference(name):
    case = sr.build_case(name, **ALL[name])
    ref, A = sr.reference(case)
    return case, ref, A


def _plan(lib, case, *, step_cached=0, pos_bound=0, all_zero=0, flags=0):
    return lib.swx_test_self_attn_plan(1 if case.f16 else 0, case.R, case.H, case.n_new, case.n_ctx, case.row_mul,
                                       1 if case.skip_append else 0, step_cached, pos_bound, all_zero, 0 if case.anc is None else 1, flags)


def _check(case, got, ref, A, kernel_id, what=""):
    ratio = sr.worst_ratio(case, got, ref, A)
    print(f"self-attn ratio kernel={kernel_id} {sr.KERNEL_NAMES[kernel_id]} case={case.name} {what} max error/tolerance = {ratio:.4f}")
    assert ratio <= 1.0, (f"{sr.KERNEL_NAMES[kernel_id]} on {case.name} {what}: largest |got - ref| / tolerance = {ratio:.4g} "
                          f"({int((~np.isfinite(np.asarray(got, np.float64))).sum())} non-finite outputs)")


def _device_inputs(case):
    kb, vb = case.caches_before()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t(case.qkv()), t(kb), t(vb), None if case.anc is None else t(case.anc), t(case.pos0)


STEP_ALL = sr.case_table(sr.step_cases(False))
STEP_SHORT = sr.case_table(sr.step_cases(True))
MULTI = sr.case_table(sr.multi_cases())
GENERAL = sr.case_table(sr.general_cases())
ALL = {**STEP_ALL, **STEP_SHORT, **MULTI, **GENERAL}


# ------------------------------------------------------------------------------------------------- single-token step
# (variant of swx_test_self_attn_step, debug flags, kernel id): the general kernel first -- the bit-identity reference of the others
STEP_LAUNCHES_ALL = ((2, 0, sr.K_CACHED_F16), (1, 0, sr.K_STEP_DEEP), (1, sr.FLAG_NO_DEEP, sr.K_STEP_LONG), (1, sr.FLAG_WG5, sr.K_STEP_LONG_WG5))
STEP_LAUNCHES_SHORT = STEP_LAUNCHES_ALL + ((0, 0, sr.K_STEP), (0, sr.FLAG_WG5, sr.K_STEP_WG5))


@pytest.mark.parametrize("name,table", [(n, "all") for n in STEP_ALL] + [(n, "short") for n in STEP_SHORT])
def test_step_kernels_against_f64(name, table):
    lib = _lib()
    case, ref, A = _case_and_reference(name)
    q, kc, vc, anc, pos = _device_inputs(case)
    kc0, vc0 = kc.clone(), vc.clone()
    old = lib.swx_debug_flags(-1)
    base = old & ~(sr.FLAG_NO_DEEP | sr.FLAG_WG5)
    general = None
    try:
        for variant, flags, kid in (STEP_LAUNCHES_ALL if table == "all" else STEP_LAUNCHES_SHORT):
            step = 1 if variant < 2 else 0
            assert _plan(lib, case, step_cached=step, pos_bound=128 if variant == 0 else 0, flags=base | flags) == kid
            o = torch.full((case.R, case.d), float("nan"), dtype=torch.half, device="cuda")
            lib.swx_debug_flags(base | flags)
            rc = lib.swx_test_self_attn_step(_p(q), _p(kc), _p(vc), _p(anc), _p(pos), case.R, case.H, case.n_ctx, case.d, variant, _p(o),
                                             _stream())
            torch.cuda.synchronize()
            lib.swx_debug_flags(old)
            assert rc == 0, (kid, rc)
            got = o.cpu().numpy()
            _check(case, got, ref, A, kid)
            if general is None:
                general = got
            assert sr.same_bits(got, general), (sr.KERNEL_NAMES[kid], "differs from the general kernel")
    finally:
        lib.swx_debug_flags(old)
    assert sr.same_bits(kc.cpu().numpy(), kc0.cpu().numpy()) and sr.same_bits(vc.cpu().numpy(), vc0.cpu().numpy())     # read-only


# ------------------------------------------------------------------------------------- multi-token, rows from position 0
@pytest.mark.parametrize("name", list(MULTI))
def test_multi_token_kernels_against_f64(name):
    lib = _lib()
    case, ref, A = _case_and_reference(name)
    q, kc, vc, _, _ = _device_inputs(case)
    n_new = case.n_new
    want_mq = sr.K_CACHED_F16 if n_new < 8 else sr.K_MQ4 if n_new < 32 else sr.K_MQ8     # 4 waves per workgroup from 8 tokens, 8 from 32
    outs = []
    for mq, kid in ((0, sr.K_CACHED_F16), (1, want_mq)):
        assert _plan(lib, case, all_zero=mq, flags=lib.swx_debug_flags(-1)) == kid
        o = torch.full((case.R * n_new, case.d), float("nan"), dtype=torch.half, device="cuda")
        rc = lib.swx_test_self_attn_multi(_p(q), _p(kc), _p(vc), case.R, case.H, n_new, case.n_ctx, case.d, mq, _p(o), _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        got = o.cpu().numpy()
        _check(case, got, ref, A, kid)
        outs.append(got)
    assert sr.same_bits(outs[0], outs[1])
    # token 0 attends to position 0 only: V[0] of its head, for every head
    assert sr.same_bits(outs[0].reshape(case.R, n_new, case.d)[:, 0], case.vc_dense[:, 0])


# ------------------------------------------------------------------------ general path: append, then attend; f16 and f32
@pytest.mark.parametrize("name", list(GENERAL))
def test_general_path_appends_and_attends_against_f64(name):
    lib = _lib()
    case, ref, A = _case_and_reference(name)
    qkv, kc, vc, anc, pos = _device_inputs(case)
    kid = sr.K_CACHED_F16 if case.f16 else sr.K_CACHED_F32
    assert _plan(lib, case, flags=lib.swx_debug_flags(-1)) == kid
    assert qkv.shape == (case.R * case.n_new, 3 * case.d) and kc.shape == (case.R * case.row_mul, case.n_ctx, case.d)
    o = torch.full((case.R * case.n_new, case.d), float("nan"), dtype=qkv.dtype, device="cuda")
    rc = lib.swx_test_self_attn_general(1 if case.f16 else 0, _p(qkv), 3 * case.d, _p(kc), _p(vc), _p(anc), _p(pos), case.R, case.H,
                                        case.n_new, case.n_ctx, case.d, case.row_mul, 0, 0, _p(o), _stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    _check(case, o.cpu().numpy(), ref, A, kid, f"row_mul={case.row_mul}")
    # the caches afterwards: the new tokens' K / V are exact copies at pos0[r] + i of row r, every other byte is as it was
    ka, va = case.caches_after()
    assert sr.same_bits(kc.cpu().numpy(), ka), "K cache"
    assert sr.same_bits(vc.cpu().numpy(), va), "V cache"


def test_general_hook_refuses_what_it_cannot_run():
    lib = _lib()
    case, _, _ = _case_and_reference("general-f16-H2-q0.8-mul1-n1-noanc")
    qkv, kc, vc, _, pos = _device_inputs(case)
    o = torch.full((case.R, case.d), float("nan"), dtype=torch.half, device="cuda")

    def call(ld=3 * case.d, H=case.H, n_ctx=case.n_ctx, d=case.d, row_mul=1, skip=0):
        return lib.swx_test_self_attn_general(1, _p(qkv), ld, _p(kc), _p(vc), None, _p(pos), case.R, H, 1, n_ctx, d, row_mul, skip, 0, _p(o),
                                              _stream())
    assert call(n_ctx=513) < 0 and call(d=case.d + 64) < 0 and call(H=case.H + 1) < 0 and call(row_mul=0) < 0
    assert call(ld=3 * case.d - 8) < 0 and call(ld=case.d - 8, skip=1) < 0 and call(ld=case.d, skip=0) < 0
    torch.cuda.synchronize()
    assert torch.isnan(o).all()                                     # nothing was launched
