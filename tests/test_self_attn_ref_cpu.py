"""Conditions on the self-attention cases and their float64 reference (tests/self_attn_ref.py), checked without a GPU:

* the reference reads no cache entry the contract does not name: it is finite on the NaN-poisoned caches;
* an f32 restatement of the same formula (rounded to the output type) is within the tolerance of the f64 reference -- the
  tolerance is not one that only an f64 computation could meet;
* every deliberately wrong statement of the contract (newest key dropped, one ancestor entry pointing at another row of the
  group, heads shifted by one, scale 0.124, V of two positions swapped) is OUTSIDE the tolerance on every case it can show on --
  otherwise the case's inputs are too bland to tell a wrong kernel from a right one;
* the dispatch: swx_test_self_attn_plan / swx_test_dec_plan name, for every GPU case of tests/test_gpu_self_attn.py and the tall
  dec GEMM cases of tests/test_gpu_kernels.py, the kernel the case is meant to run (host-only queries: no GPU).
"""
import numpy as np
import pytest

import self_attn_ref as sr

CASES = sr.case_table(sr.all_cases())


def _applicable(case, mutation):
    keys = int(case.pos0[::case.row_mul].max()) + case.n_new         # keys of the row with the most
    if mutation == "wrong_ancestor":
        return case.rows_phys > 1 and keys >= 2                      # a single cache row has no other row to read
    if mutation in ("scale_0.124", "swap_v"):
        return keys >= 2                                             # a softmax over one key is 1 whatever the score
    return True


@pytest.mark.parametrize("name", list(CASES))
def test_reference_tolerance_and_mutations(name):
    case = sr.build_case(name, **CASES[name])
    ref, A = sr.reference(case)                                      # asserts finiteness on the poisoned caches
    dense, _ = sr.attention(case, case.kc_dense, case.vc_dense)
    assert np.array_equal(dense, ref)                                # ... and the unreferenced entries do not enter it
    kb, vb = case.caches_before()
    ka, va = case.caches_after()
    keep0 = np.zeros_like(case.referenced)
    keep0[np.arange(case.R) * case.row_mul, 0] = True
    assert np.isnan(kb[~case.referenced & ~keep0]).all() and np.isnan(vb[~case.referenced & ~keep0]).all()
    assert np.isfinite(ka[case.referenced | keep0]).all() and np.isfinite(va[case.referenced | keep0]).all()
    if not case.skip_append:
        assert np.isnan(kb[case.appended]).all() and case.qkv().shape[1] == 3 * case.d
    emu, _ = sr.attention(case, case.kc_dense, case.vc_dense, np.float32)
    r_emu = sr.worst_ratio(case, emu.astype(case.dtype), ref, A)
    assert r_emu <= 1.0, r_emu
    for mutation in sr.MUTATIONS:
        if not _applicable(case, mutation):
            continue
        wrong, _ = sr.attention(case, case.kc_dense, case.vc_dense, mutate=mutation)
        ratio = sr.worst_ratio(case, wrong, ref, A)
        assert ratio > 1.0, (mutation, ratio)


def test_every_mutation_is_exercised_by_most_cases():
    counts = {m: 0 for m in sr.MUTATIONS}
    for name, kw in CASES.items():
        pos0, n_new, rows = kw["pos0"], kw["n_new"], len(kw["pos0"]) * kw.get("row_mul", 1)
        keys = max(pos0) + n_new
        for m in sr.MUTATIONS:
            ok = (rows > 1 and keys >= 2) if m == "wrong_ancestor" else keys >= 2 if m in ("scale_0.124", "swap_v") else True
            counts[m] += ok
    # (the one-row and the one-key cases of the multi-token list: per geometry its R = 1 half and the n_new = 1 case of its R = 3 half)
    excused = len(sr.GEOMETRIES) * (len(sr.MULTI_N_NEW) + 1)
    assert all(c >= len(CASES) - excused for c in counts.values()), counts


# ------------------------------------------------------------------------------------------------- dispatch, host-only
@pytest.fixture(scope="module")
def lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _sa_plan(lib, *, f16=True, R, H, n_new, row_mul=1, skip_append=1, step_cached=0, pos_bound=0, all_zero=0, anc=0, flags=0, n_ctx=sr.N_CTX):
    return lib.swx_test_self_attn_plan(1 if f16 else 0, R, H, n_new, n_ctx, row_mul, skip_append, step_cached, pos_bound, all_zero, anc, flags)


@pytest.mark.parametrize("H", [2, 6])
@pytest.mark.parametrize("anc", [0, 1])
def test_plan_of_the_step_cases(lib, H, anc):
    R, Rs = len(sr.STEP_POSITIONS), len(sr.STEP_POSITIONS_SHORT)
    assert R % 5 and Rs % 5                                                       # the five-row forms get a ragged last workgroup
    for rows in (R, Rs):
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc) == sr.K_CACHED_F16
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc, step_cached=1) == sr.K_STEP_DEEP
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc, step_cached=1, flags=sr.FLAG_NO_DEEP) == sr.K_STEP_LONG
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc, step_cached=1, flags=sr.FLAG_WG5) == sr.K_STEP_LONG_WG5
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc, step_cached=1, pos_bound=128) == sr.K_STEP
        assert _sa_plan(lib, R=rows, H=H, n_new=1, anc=anc, step_cached=1, pos_bound=128, flags=sr.FLAG_WG5) == sr.K_STEP_WG5


def test_plan_thresholds(lib):
    # R x H <= 1024 waves and n_ctx <= 448: the two-batch kernel; bound <= 128: the short kernel
    assert _sa_plan(lib, R=51, H=20, n_new=1, step_cached=1) == sr.K_STEP_DEEP
    assert _sa_plan(lib, R=52, H=20, n_new=1, step_cached=1) == sr.K_STEP_LONG
    assert _sa_plan(lib, R=5, H=20, n_new=1, step_cached=1, n_ctx=449) == sr.K_STEP_LONG
    assert _sa_plan(lib, R=5, H=20, n_new=1, step_cached=1, pos_bound=129) == sr.K_STEP_DEEP
    assert _sa_plan(lib, R=5, H=20, n_new=1, step_cached=1, pos_bound=1) == sr.K_STEP
    # the step kernels are f16, one token, row_mul 1, K / V appended already; n_ctx <= 512 everywhere
    assert _sa_plan(lib, f16=False, R=5, H=20, n_new=1, step_cached=1) < 0
    assert _sa_plan(lib, R=5, H=20, n_new=2, step_cached=1) < 0
    assert _sa_plan(lib, R=5, H=20, n_new=1, step_cached=1, row_mul=5) < 0
    assert _sa_plan(lib, R=5, H=20, n_new=1, step_cached=1, skip_append=0) < 0
    assert _sa_plan(lib, R=5, H=20, n_new=1, n_ctx=513) < 0 and _sa_plan(lib, R=5, H=20, n_new=1, n_ctx=512) == sr.K_CACHED_F16


@pytest.mark.parametrize("n_new", sr.MULTI_N_NEW)
@pytest.mark.parametrize("R", [1, 3])
def test_plan_of_the_multi_token_cases(lib, R, n_new):
    want = sr.K_CACHED_F16 if n_new < 8 else sr.K_MQ4 if n_new < 32 else sr.K_MQ8
    for H in (2, 6):
        assert _sa_plan(lib, R=R, H=H, n_new=n_new, all_zero=1) == want
        assert _sa_plan(lib, R=R, H=H, n_new=n_new, all_zero=0) == sr.K_CACHED_F16
        assert _sa_plan(lib, R=R, H=H, n_new=n_new, all_zero=1, anc=1) == sr.K_CACHED_F16
        assert _sa_plan(lib, R=R, H=H, n_new=n_new, all_zero=1, flags=256) == sr.K_CACHED_F16
        assert _sa_plan(lib, f16=False, R=R, H=H, n_new=n_new, all_zero=1) == sr.K_CACHED_F32


def test_plan_of_the_general_cases(lib):
    for name, kw in sr.general_cases():
        got = _sa_plan(lib, f16=kw["f16"], R=len(kw["pos0"]), H=kw["H"], n_new=kw["n_new"], row_mul=kw["row_mul"], skip_append=0,
                       anc=int(kw["use_anc"]))
        assert got == (sr.K_CACHED_F16 if kw["f16"] else sr.K_CACHED_F32), name


# tall dec GEMM cases of tests/test_gpu_kernels.py: (M, N, K, epilogue) with LN 1, GELU 2, RES 4, QKV 8, SLAB 16; 64 = a multi-token pass
DEC_W4, DEC_W1, DEC_TALL4, DEC_TALL8 = range(4)
TALL_M = (161, 176, 177, 333)
TALL_NKE = ((384, 384, 1), (1152, 384, 1 | 8), (1536, 384, 1 | 2), (384, 384, 4), (384, 1536, 4 | 16))
TALL_W8 = ((200, 3072, 1024, 1 | 8), (161, 1280, 5120, 4 | 16))
NO_TALL, TALL_NO_W8 = 524288, 32


def test_plan_of_the_tall_dec_gemm_cases(lib):
    plan = lib.swx_test_dec_plan
    for M in TALL_M:
        for N, K, epi in TALL_NKE:
            assert plan(M, N, K, epi | 64, 0) == DEC_TALL4, (M, N, K, epi)
            assert plan(M, N, K, epi | 64, NO_TALL) in (DEC_W4, DEC_W1), (M, N, K, epi)
            assert plan(M, N, K, epi, 0) in (DEC_W4, DEC_W1), (M, N, K, epi)          # not a multi-token pass: never tall
    for M, N, K, epi in TALL_W8:
        assert plan(M, N, K, epi | 64, 0) == DEC_TALL8
        assert plan(M, N, K, epi | 64, TALL_NO_W8) == DEC_TALL4
        assert plan(M, N, K, epi | 64, NO_TALL) == DEC_W4
    # the thresholds: more than 160 rows; eight waves from 40 (panel, K slice) units, an even panel count, K slices of whole 256s
    assert plan(160, 384, 384, 1 | 64, 0) in (DEC_W4, DEC_W1) and plan(161, 384, 384, 1 | 64, 0) == DEC_TALL4
    assert plan(200, 2560, 1024, 1 | 64, 0) == DEC_TALL8 and plan(200, 2432, 1024, 1 | 64, 0) == DEC_TALL4      # 40 / 38 panels
    assert plan(200, 3072, 768, 1 | 64, 0) == DEC_TALL8 and plan(200, 3072, 384, 1 | 64, 0) == DEC_TALL4        # 24 / 12 k-steps
    assert plan(200, 1280, 1280, 4 | 64, 0) == DEC_TALL4                                                       # 20 units
    # decode-step sized launches: single-wave workgroups up to 80 four-wave workgroups of one row tile
    assert plan(5, 1280, 1280, 4, 0) == DEC_W1 and plan(5, 1280, 1280, 4, 16) == DEC_W4
    assert plan(5, 5120, 1280, 1 | 2, 0) == DEC_W1 and plan(100, 5120, 1280, 1 | 2, 0) == DEC_W4
    assert plan(5, 1000, 1280, 4, 0) < 0 and plan(5, 1280, 1000, 4, 0) < 0


def test_plan_of_the_single_wave_row_staging_cases(lib):
    # test_dec_gemm_single_wave_partial_tile_staging_is_bit_identical (tests/test_gpu_kernels.py): every launch of it is the single-wave
    # kernel, with the row-staging switch (1024) off and on; the switch is not the multi-token self-attention's (256) any more
    plan = lib.swx_test_dec_plan
    for N, K in ((384, 384), (1280, 1280), (3840, 1280), (1280, 5120)):
        epis = [4 | 16] + ([1, 1 | 2] if K <= 1280 else []) + ([1 | 8] if N == 3 * K else [])
        for M in (1, 5, 15, 16):
            for epi in epis:
                assert plan(M, N, K, epi, 0) == DEC_W1 and plan(M, N, K, epi, 1024) == DEC_W1, (M, N, K, epi)
                assert plan(M, N, K, epi, 16) == DEC_W4, (M, N, K, epi)
