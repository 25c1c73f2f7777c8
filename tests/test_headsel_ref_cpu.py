"""Conditions on the head-selection cases and their float64 reference (tests/headsel_ref.py), checked without a GPU:

* the reference reads nothing the contract does not name: it is finite on the NaN-poisoned q and K, and equal to what it computes
  from the dense arrays;
* the inputs can tell heads and frames apart: the gap conditions of headsel_ref.violations hold, the planted exact ties are
  where the case says they are and nowhere else, and planted heads win (past head 256 too in the wide configuration);
* an f32 restatement of the same formulas is within a QUARTER of every tolerance -- the tolerances are not ones only an f64
  computation could meet, and leave the kernels' block-tree sums and expf a factor of four;
* every deliberately wrong statement of the contract (headsel_ref.MUTATIONS) is OUTSIDE the tolerance of at least one compared
  quantity on every case it can show on;
* the layout hook: swx_test_heads_layout reports ascending, non-overlapping regions whose total is what the scratch-size queries
  return (host-only calls: no GPU).
"""
import ctypes

import numpy as np
import pytest

import headsel_ref as hr

CASES = hr.case_table(hr.all_cases())


def _applicable(kw, mutation):
    """whether a wrong statement changes anything the case compares (kw: the case's builder arguments)"""
    if kw["kind"] == "dynamic":
        if mutation == "peak_highest_on_tie":
            return bool(kw.get("frame_tie"))                          # without two equal maxima both rules name the same frame
        if mutation == "peaks_without_midpoint":
            return kw.get("peaks") == "mid"
        if mutation == "score_without_qk_scale":
            return kw.get("qk_scale", 1.0) != 1.0
        if mutation == "softmax_all_frames":
            return min(kw["frames"]) < hr.N_AUDIO_CTX
        if mutation == "k_of_previous_window":
            return len(kw["rows"]) > 1
        return True
    width, pad = kw.get("width", 7), kw.get("width", 7) // 2
    if mutation in ("median_after_softmax", "symmetric_padding"):
        return width > 1 and max(kw["frames"]) > pad                  # a pass-through filter commutes with everything
    if mutation == "crop_after_median":
        return width > 1 and min(kw["frames"]) < hr.N_AUDIO_CTX
    if mutation == "rownorm_without_sqrt":
        return kw.get("w_row", 1.0) > 0
    if mutation in ("coverage_without_clamp", "coverage_without_half_F"):
        return kw.get("w_cov", 0.0) > 0
    if mutation == "mean_over_LH":
        return kw.get("topk", 20) != (264 if kw.get("wide") else 24)
    return True


def _check_ties(case, ref):
    """the planted ties are in the compared ranks, and decided the documented way"""
    if "frames" in case.ties:
        w, f1, f2 = case.ties["frames"]
        z, sel = ref["logits"][w], ref["sel"][w]
        hit = [(h, i) for i in range(case.rows(w)) for h in sel[i] if z[h, i, f1] == z[h, i, f2] == z[h, i].max()]
        assert hit, "no picked head has its maximum on the two equal frames"
        wrong = hr.compute(case, mutate="peak_highest_on_tie")
        assert all(wrong["dscore"][w][h, i] != ref["dscore"][w][h, i] for h, i in hit)
    for a, b in case.ties.get("heads", ()):
        assert a < 256 <= b
        for w in range(case.W):
            if case.kind == "dynamic":
                assert np.array_equal(ref["dscore"][w][a], ref["dscore"][w][b])
                for row in ref["sel"][w]:
                    ia, = np.nonzero(row == a)
                    assert ia.size == 1 and row[ia[0] + 1] == b, (w, row, a, b)      # both in the compared ranks, the lower first
            else:
                assert ref["nscore"][w][a] == ref["nscore"][w][b]
                ia, = np.nonzero(ref["top"][w] == a)
                assert ia.size == 1 and ref["top"][w][ia[0] + 1] == b, (w, ref["top"][w], a, b)
    for w in case.ties.get("one_frame", ()):
        assert case.n_frames[w] == 1 and (ref["nscore"][w] == ref["nscore"][w][0]).all()
        assert np.array_equal(ref["top"][w], np.arange(case.opts["topk"]))


@pytest.mark.parametrize("name", list(CASES))
def test_reference_conditions_tolerances_and_mutations(name):
    kw = CASES[name]
    case = hr.get_case(name)
    assert case.max_n <= 24 and case.W <= 3
    ref = hr.reference(case)                                              # asserts finiteness on the poisoned inputs
    dense = hr.compute(case)
    q, k = case.poisoned()
    for w in range(case.W):
        assert np.isnan(q[:, w, case.n_tok[w]:]).all() and np.isnan(k[:, w, case.n_frames[w]:]).all()
        assert np.isfinite(q[:, w, :case.n_tok[w]]).all() and np.isfinite(k[:, w, :case.n_frames[w]]).all()
    # ... and the poisoned entries do not enter it (the two differ by f64 rounding: the matrix products run over other strides)
    assert max(hr.worst_ratios(case, dense, ref).values()) <= 1e-6
    assert hr.violations(case, ref) == []
    _check_ties(case, ref)
    picks = ref["sel" if case.kind == "dynamic" else "top"]
    won = [set(np.asarray(p).ravel().tolist()) & set(pl) for p, pl in zip(picks, case.planted)]
    if kw.get("wide"):
        assert all(any(h >= 256 for h in s) and any(h < 256 for h in s) for s in won), won
    elif max(case.n_frames) >= 64 and case.opts.get("topk", 2) > 1:
        assert any(won), won
    emu = hr.compute(case, dtype=np.float32)
    for quantity, r in hr.worst_ratios(case, emu, ref).items():
        assert r <= 0.25, (quantity, r)
    for mutation in hr.MUTATIONS[case.kind]:
        if not _applicable(kw, mutation):
            continue
        ratios = hr.worst_ratios(case, hr.compute(case, mutate=mutation), ref)
        assert max(ratios.values()) > 1.0, (mutation, ratios)
        if mutation == "coverage_without_half_F":                         # a constant off every head's score: nothing else moves
            assert ratios["nscore"] > 1.0 and ratios["top"] == 0.0 and max(ratios["matrix"], ratios["colnorm"]) <= 1e-6, ratios


def test_every_mutation_is_exercised_by_most_cases():
    for kind, mutations in hr.MUTATIONS.items():
        cases = [kw for kw in CASES.values() if kw["kind"] == kind]
        counts = {m: sum(_applicable(kw, m) for kw in cases) for m in mutations}
        # the special cases: the frame tie, the previous pass's midpoints, qk_scale = 2, a coverage weight -- one or a few cases each
        few = {"peak_highest_on_tie": 2, "peaks_without_midpoint": 6, "score_without_qk_scale": 4, "coverage_without_clamp": 2,
               "coverage_without_half_F": 2}
        for m, c in counts.items():
            assert c >= few.get(m, len(cases) - 4), (m, c, len(cases))


@pytest.mark.parametrize("n_in", hr.POOL_N_IN)
def test_pool_restatement(n_in):
    for n in hr.POOL_SIZES[:3]:
        coef, xs = hr.pool_inputs(n_in, n)
        ref, mag = hr.pool(coef, xs)
        emu, _ = hr.pool(coef, xs, np.float32)
        assert hr.ratio(emu, ref, hr.tol_pool(n_in, mag)) <= 0.25
        if n_in > 1:
            wrong, _ = hr.pool(coef[::-1], xs)
            assert hr.ratio(wrong, ref, hr.tol_pool(n_in, mag)) > 1.0


# ------------------------------------------------------------------------------------------------- the layout hook, host-only
@pytest.fixture(scope="module")
def lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _handle(lib, L, H, f16):
    from stable_ts_amd._lib import swx_dims
    dims = swx_dims(n_mels=80, n_audio_ctx=1500, n_audio_state=384, n_audio_head=6, n_audio_layer=4, n_vocab=51865, n_text_ctx=448,
                    n_text_state=64 * H, n_text_head=H, n_text_layer=L)
    h = ctypes.c_void_p()
    assert lib.swx_model_create(ctypes.byref(dims), 1 if f16 else 0, ctypes.byref(h)) == 0
    return h


@pytest.mark.parametrize("L,H", [(4, 6), (44, 6)])
def test_heads_layout_hook(lib, L, H):
    h = _handle(lib, L, H, True)
    LH = L * H
    try:
        for W, max_n, count in ((1, 5, 1), (2, 17, 4), (3, 24, 24), (3, 9, 0), (0, 5, 0), (0, 24, 7)):
            out = (ctypes.c_int64 * 9)()
            assert lib.swx_test_heads_layout(h, W, max_n, count, out) == 0
            cnt, score, sel, colnorm, nscore, top, gathered, rstat, total = list(out)
            want = lib.swx_heads_batch_scratch_bytes(h, W, max_n, count) if W else lib.swx_heads_scratch_bytes(h, max_n)
            assert total == want > 0
            w = max(W, 1)
            sizes = [3 * 4 * W, w * LH * max_n * 8, (w * max_n * max(count, 1) if W else LH * max_n) * 4, w * LH * hr.HS_MAXF * 4,
                     w * LH * 4, w * LH * 4, W * count * max_n * hr.N_AUDIO_CTX * 4, W * count * max_n * 8]
            offs = [cnt, score, sel, colnorm, nscore, top, gathered, rstat, total]
            assert offs[0] == 0 and all(o % 256 == 0 for o in offs)
            for k, size in enumerate(sizes):                              # ascending, every region fits before the next begins
                assert offs[k] + size <= offs[k + 1], (W, max_n, count, k)
        bad = (ctypes.c_int64 * 9)()
        assert lib.swx_test_heads_layout(h, -1, 5, 1, bad) < 0 and lib.swx_test_heads_layout(h, 1, 0, 1, bad) < 0
        assert lib.swx_test_heads_layout(None, 1, 5, 1, bad) < 0
    finally:
        lib.swx_model_destroy(h)
