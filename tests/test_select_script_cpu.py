"""Conditions on the scripted selection cases (tests/select_script.py), checked on the reference alone -- no GPU:

* every decision margin the reference measures in float64 is at least 1e-3 (100 times the f32 log-softmax error at the
  magnitudes used), so the kernels' f32 arithmetic cannot legitimately decide otherwise; planted exact ties are excepted, they
  are bit-equal on both sides; the margin of a draw by the built-in hashed sampler is measured after every key has given up its
  distance to the neighbouring buckets' variates (the device's f32 variate may sit one bucket off in the far tails);
* finite scripted logits lie in [-20, 20] (the sum_logprobs tolerance of the GPU test is worked out for that);
* over the whole case list every rule branch the GPU test is meant to reach is reached at least once;
* the helper follows ``_main_loop``: fed the logits a small real decoder produced, it reproduces ``oracle.stable.decode_stable``.
"""
from collections import Counter

import numpy as np
import pytest
import torch

import select_script as ss

BRANCHES = [
    "pair_ts_ts", "pair_text_ts", "hist_ts_text", "no_timestamp_yet", "repeat_allowed", "repeat_forbidden",
    "mono_tl", "mono_tl_plus_1", "text_suppressed", "text_kept", "ts_mass_beats_single_text", "ts_mass_loses",
    "max_initial_cut", "ts_mask", "ts_mask_strikes_whole_row", "poll_exit", "nan_text", "nan_ts", "pinf_text", "pinf_ts", "ninf_text", "ninf_ts", "compare_nonfinite",
    "suppress_blank", "blank_allowed_later", "suppress_list", "min_tokens_on", "min_tokens_lifted",
    "early_window_freeze", "steps_past_completion", "row_past_eot", "beam_finished", "patience_max_cand", "max_cand_overflow",
    "finalize_top_up", "unused_slot", "ctx_full_ragged", "ctx_full_uniform",
]


@pytest.fixture(scope="module")
def survey():
    """one pass over all cases: (name, smallest margin, its label, steps) per case and the branch counters of the whole list"""
    rows, total, names = [], Counter(), []
    for make in ss.all_cases():
        case = make()
        for a in (case.prefill, case.script):
            fin = a[np.isfinite(a)]
            assert fin.min() >= -20 and fin.max() <= 20, case.name
        M = case.W * case.G
        assert 12 <= case.n_ctx <= 24 and case.sample_len <= 24 and M <= 10, case.name
        assert case.script.shape == (case.script.shape[0], M, case.V) and case.prefill.shape == (case.W, 2, case.V)
        ref = ss.run_reference(case)
        assert ref.steps - 1 <= case.script.shape[0], case.name
        worst = min(ref.margins, key=lambda m: m[3]) if ref.margins else None
        rows.append((case.name, worst, ref))
        total.update(ref.counts)
        names.append(case.name)
    assert len(set(names)) == len(names)
    return rows, total


def test_every_decision_margin_is_wide(survey):
    rows, _ = survey
    bad = [(name, worst) for name, worst, _ in rows if worst is not None and not worst[3] >= ss.MARGIN]
    assert not bad, bad


def test_every_branch_is_reached(survey):
    _, total = survey
    missing = [b for b in BRANCHES if total[b] == 0]
    assert not missing, (missing, dict(total))


def test_layouts_and_kinds_are_all_present(survey):
    rows, _ = survey
    names = [n for n, _, _ in rows]
    for V in ss.LAYOUTS:
        mine = [n for n in names if n.endswith(f"_V{V}")]
        assert any(n.startswith("ties") for n in mine) and any(n.startswith("beam") for n in mine) and \
            any(n.startswith("rules") for n in mine), (V, mine)
    for V in ss.RULE_LAYOUTS:
        mine = [n for n in names if n.endswith(f"_V{V}")]
        for kind in ("rules_mi-1", "rules_mi0", "rules_mi50", "filters", "ts_mask_pick", "ts_mask_all", "nonfinite_nan",
                     "nonfinite_pinf", "nonfinite_ninf", "nonfinite_all", "greedy_eot", "sampling", "hashed_T0.2_V", "hashed_T1.0_V",
                     "hashed_T1.0_uid", "top_bucket_suppressed", "top_bucket_far_below", "beam_a_G2_p1.0",
                     "beam_b_G5_p1.0", "beam_c_G5_p1.0", "beam_c_G2_p2.0", "beam_b_G2_p2.0", "beam_b_G5_p2.0", "ragged",
                     "poll_exit", "ctx_exact", "beam_ctx"):
            assert any(n.startswith(kind) for n in mine), (V, kind)


def test_expected_outcomes_of_the_planted_cases(survey):
    """the scripts do what their docstrings say (on the reference): spot checks that pin the case list against silent decay"""
    by = {n: r for n, _, r in survey[0]}
    for V in ss.RULE_LAYOUTS:
        tok = ss.Tok(V)
        tsb = tok.timestamp_begin
        r = by[f"rules_mi-1_V{V}"]
        got = r.tokens[0, 0, 3:3 + r.lens[0, 0]].tolist()
        assert got[0] == tsb + 60 and got[3] == got[4] == tsb + 70 and got[6] < tsb <= got[7] and len(got) == 8, got
        assert by[f"rules_mi0_V{V}"].tokens[0, 0, 3] == tsb and by[f"rules_mi50_V{V}"].tokens[0, 0, 3] == tsb + 10
        r = by[f"greedy_eot_V{V}"]
        assert r.lens[:, 0].tolist() == [2, 11] and r.steps == 11
        r = by[f"sampling_V{V}"]
        assert sorted(r.lens[0].tolist()) == [1, 3, 6] and r.tokens[0, 1, 4] == 81 and r.tokens[0, 0, 4] == 80
        r = by[f"ragged_V{V}"]
        assert r.lens[:, 0].tolist() == [10, 4] and r.steps == 10 and r.pos0.tolist() == [11, 11]
        r = by[f"poll_exit_V{V}"]
        assert r.lens[:, 0].tolist() == [1, 3] and r.steps == 8
        # ts mask with the rules on: the favourite (+400) and the mask's last entry (+1500) are struck, +410 is left; with every
        # timestamp masked the text is still struck on the timestamps' mass and index 0 wins the all-equal row
        r = by[f"ts_mask_pick_V{V}"]
        assert r.tokens[:, 0, 3:8].tolist() == [[tsb + 10, 30, 31, tsb + 410, tsb + 500], [tsb + 10, 30, 31, tsb + 1500, tok.eot]]
        r = by[f"ts_mask_all_V{V}"]
        assert r.tokens[0, 0, 3:8].tolist() == [0, 30, 31, 0, 33]
        r = by[f"ctx_exact_V{V}"]
        assert r.steps == 9 and r.lens[0, 0] == 9 and r.pos0.tolist() == [11]
        r = by[f"beam_b_G2_p2.0_V{V}"]
        assert r.lens[0].tolist().count(-1) == 2
        # the hashed sampler's top bucket on a token that must not win: the lead is selected at that very (step, row)
        for kind in ("suppressed", "far_below"):
            c = ss.case_top_bucket(V, kind == "suppressed")
            step, row, x = c.planted
            assert step <= 4 and ss.sampler_ref.bucket(ss.sampler_ref.words(c.seed, row, step, x)) == (1 << 24) - 1
            r = by[f"top_bucket_{kind}_V{V}"]
            assert r.tokens[row // c.G, row % c.G, 4 + step] == 300 + (step & 1) != x
            assert (x in c.suppress) == (kind == "suppressed") and c.noise is None and c.seed >> 32 and c.seed & 0xFFFFFFFF
            if kind == "far_below":
                assert c.logits(row // c.G, step)[row % c.G, x] == ss.LEAD - 30.0 and c.logits(row // c.G, step)[row % c.G].max() == ss.LEAD
        # NaN in the text range: the reference keeps the text tokens (its log-softmax is NaN everywhere) and picks the best one
        r = by[f"nonfinite_nan_V{V}"]
        assert r.tokens[0, 0, 6] == 32 and r.tokens[1, 0, 6] == 32 and r.tokens[2, 0, 6] == 32


def test_helper_follows_main_loop_on_a_real_decoder(monkeypatch):
    """logits recorded from a small decoder while oracle.stable.decode_stable runs, replayed through the helper"""
    from oracle import stable as ost
    from oracle.whisper import decoding as od
    from oracle.whisper import model as om
    V = 51864
    dims = om.ModelDimensions(80, 24, 64, 2, 1, V, 24, 64, 2, 1)
    torch.manual_seed(5)
    model = om.Whisper(dims).eval()
    with torch.no_grad():
        model.decoder.token_embedding.weight.mul_(3.0)
    feats = torch.randn(1, dims.n_audio_ctx, dims.n_audio_state)
    opts = od.DecodingOptions(fp16=False, language="en", sample_len=10, max_initial_timestamp=None)
    seen = []
    plain = od.PyTorchInference.logits

    def recording(self, tokens, audio_features):
        out = plain(self, tokens, audio_features)
        seen.append(out.detach().clone())
        return out
    monkeypatch.setattr(od.PyTorchInference, "logits", recording)
    want, _ = ost.decode_stable(model, feats[0], opts, min_tokens=6)
    task = ost.DecodingTaskStable(model, opts)
    tk = task.tokenizer
    stub = ss.Tok(V)
    assert (stub.eot, stub.sot, stub.no_timestamps, stub.no_speech, stub.timestamp_begin) == \
        (tk.eot, tk.sot, tk.no_timestamps, tk.no_speech, tk.timestamp_begin)
    n0 = len(task.initial_tokens)
    prefill = np.stack([seen[0][0, task.sot_index].numpy(), seen[0][0, -1].numpy()])[None]
    script = np.stack([s[:, -1].numpy() for s in seen[1:]]) if len(seen) > 1 else np.zeros((0, 1, V), np.float32)
    case = ss.Case("real", V, dims.n_text_ctx, 1, 1, 10, [list(task.initial_tokens)], prefill.astype(np.float32),
                   script.astype(np.float32), suppress_blank=1, rules=1, suppress=tuple(task._get_suppress_tokens()), min_tokens=6,
                   blank=tk.encode(" ")[0])
    ref = ss.run_reference(case)
    got = ref.tokens[0, 0, n0:n0 + ref.lens[0, 0]].tolist()
    assert got == want.tokens and len(got) >= 6
    assert abs(ref.sumlp[0, 0] / (len(got) + 1) - want.avg_logprob) < 1e-6
    assert np.isclose(ref.nospeech[0], want.no_speech_prob, rtol=0, atol=1e-7, equal_nan=True)
