"""The device paths of ``refine(batch_size=N)`` on hardware, through the C ABI, before the product drives them:

* ``swx_forward_token_ranks`` against ``swx_forward_logits`` on the same inputs (tiny.en and base.en, f32 and f16, ragged token
  counts, W = 6 and W = 2): the rank must be EXACTLY the (logit, index) count made on the host from the device's own logits;
  the probability is compared with the float64 softmax of those logits, and may deviate at most twice as far as the
  token probabilities of the existing ``swx_score`` deviate from the same float64 values on the same rows (same arithmetic,
  another launch);
* batch invariance: windows 2k, 2k + 1 of the W = 6 call are bit-identical (probability and rank) to the W = 2 call on them (two windows span
  several 64-row chunks of the vocabulary projection); the probabilities equal ``swx_score``'s bit for bit;
* ``swx_log_mel_ragged_grouped``: group = 1 and group = B are bit-identical to ``swx_log_mel_ragged`` with per_item_max 1 / 0, and with
  group = 2, B = 6 every pair is bit-identical to a B = 2, per_item_max = 0 call on that pair.

Exit code 0 = all hold.  ``--report PATH`` writes the figures as JSON (profiles/refine_lockstep_report.json is one such run).

    python tests/hw_checks/refine_lockstep_check.py [--report PATH]            (needs a GPU; run by tests/test_gpu_refine_lockstep.py in a subprocess)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "golden"))

N_TEXT = (12, 150, 7, 55, 70, 40)                # text tokens per window (ragged; two of them span several 64-row chunks)
SECONDS = (3.0, 11.5, 6.25, 9.0, 4.4, 14.0)      # audio per window (ragged)


def check(name: str, dtype: str, report: dict) -> bool:
    import stable_ts_amd as sw
    from make_golden import synth_audio
    from stable_ts_amd.refiner import token_rank
    from stable_ts_amd.tokenizer import get_tokenizer
    dims = sw.dims_for(name)
    model = sw.Whisper(dims, dtype=dtype, max_windows=6, max_rows=6)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
    eng = model.engine
    if eng.n_alignment_heads == 0:
        eng.set_alignment_heads([(dims.n_text_layer - 1, 0)])
    tok = get_tokenizer(False, num_languages=model.num_languages)
    sot = list(tok.sot_sequence)
    n_sot, eot = len(sot), tok.eot
    rng = np.random.default_rng(11)
    ids = [[*sot, tok.no_timestamps, *rng.integers(0, eot, n).tolist(), eot] for n in N_TEXT]
    audio = synth_audio(60.0, 5)
    clips, at = [], 0
    for s in SECONDS:
        n = int(s * 16000)
        clips.append(audio[at: at + n])
        at += n
    ok = True
    rep = report.setdefault(f"{name}/{dtype}", {})

    # ---- grouped log-mel.  The check that can fail is the third: every pair of a group = 2, B = 6 call against a B = 2 call of the
    # batched form.  The first two only pin the wrapper's argument mapping (swx_log_mel_ragged IS the grouped entry point with
    # group = 1 / B); that the old entry point kept its bits rests on the kernel (a max over the same per-window maxima) and on
    # tests/test_gpu_kernels.py's mel checks against the oracle.
    mel6 = model.log_mel_segments(clips, group=2)
    rep["mel_group1_is_per_item"] = bool(torch.equal(model.log_mel_segments(clips, group=1), model.log_mel_segments(clips)))
    rep["mel_groupB_is_batch_max"] = bool(torch.equal(model.log_mel_segments(clips, group=6),
                                                      model.log_mel_segments(clips, batch_max=True)))
    pair_mels = [model.log_mel_segments(clips[2 * k: 2 * k + 2], batch_max=True) for k in range(3)]
    rep["mel_pairs_are_b2_calls"] = all(bool(torch.equal(mel6[2 * k: 2 * k + 2], pair_mels[k])) for k in range(3))
    ok &= rep["mel_group1_is_per_item"] and rep["mel_groupB_is_batch_max"] and rep["mel_pairs_are_b2_calls"]

    # ---- probability and rank against the device's own logits
    xkv6 = model.cross_kv(model.encoder(mel6))
    logits = eng.forward_logits(xkv6, ids).cpu().numpy()
    prob, rank = eng.forward_token_ranks(xkv6, ids, n_vocab_used=eot)
    prob, rank = prob.cpu().numpy(), rank.cpu().numpy()
    n_frames = [min(1500, int(s * 16000) // 320 + 1) for s in SECONDS]
    score_p, _, T = eng.score(xkv6, ids, n_frames, n_sot, eot)
    rank_bad = outside_bad = rows = score_bits_differ = 0
    err_new = err_score = 0.0
    for w, t in enumerate(ids):
        for j in range(len(t) - 1):
            x, target = logits[w, j, :eot], t[j + 1]
            if target >= eot:                                    # <|notimestamps|> and the final <|endoftext|>: outside the text vocabulary
                outside_bad += not (prob[w, j] == 0.0 and rank[w, j] == -1)
                continue
            rows += 1
            rank_bad += int(rank[w, j]) != token_rank(x, target)
            x64 = x.astype(np.float64)
            want = float(np.exp(x64[target] - x64.max()) / np.exp(x64 - x64.max()).sum())
            err_new = max(err_new, abs(float(prob[w, j]) - want) / want)
            i = j - n_sot
            assert 0 <= i < T[w]
            err_score = max(err_score, abs(float(score_p[w][i]) - want) / want)
            score_bits_differ += float(prob[w, j]) != float(score_p[w][i])      # one kernel, two instantiations: the same f32
    rep.update(rows=rows, rank_mismatches=int(rank_bad), prob_differs_from_swx_score=int(score_bits_differ), outside_vocabulary_mismatches=int(outside_bad),
               prob_max_rel_err_vs_f64=err_new, swx_score_max_rel_err_vs_f64=err_score, prob_allowed=2 * err_score,
               untouched_tail_ok=bool(all((prob[w, len(t) - 1:] == 0).all() and (rank[w, len(t) - 1:] == -1).all()
                                          for w, t in enumerate(ids))))
    print(f"{name}/{dtype}: {rows} rows, rank mismatches {rank_bad}, prob max rel err {err_new:.3e} "
          f"(swx_score {err_score:.3e}, allowed {2 * err_score:.3e})", flush=True)
    ok &= rank_bad == 0 and outside_bad == 0 and score_bits_differ == 0 and err_new <= 2 * err_score and rep["untouched_tail_ok"]

    # ---- batch invariance: the pair alone (its own mel, encoder, cross-K/V, pass) == the pair inside the W = 6 call
    same = []
    for k in range(3):
        xkv2 = model.cross_kv(model.encoder(pair_mels[k]))
        p2, r2 = eng.forward_token_ranks(xkv2, ids[2 * k: 2 * k + 2], n_vocab_used=eot)
        p2, r2 = p2.cpu().numpy(), r2.cpu().numpy()
        for i in range(2):
            n = len(ids[2 * k + i]) - 1
            same.append(bool(np.array_equal(p2[i, :n].view(np.uint32), prob[2 * k + i, :n].view(np.uint32)) and
                             np.array_equal(r2[i, :n], rank[2 * k + i, :n])))
    rep["window_of_w6_equals_w2"] = same
    print(f"{name}/{dtype}: W=6 windows bit-identical to their W=2 calls: {same}", flush=True)
    ok &= all(same)
    del model
    torch.cuda.empty_cache()
    return bool(ok)


def main() -> int:
    report = {}
    ok = True
    for name in ("tiny.en", "base.en"):
        for dtype in ("f32", "f16"):
            ok &= check(name, dtype, report)
    if "--report" in sys.argv:
        path = os.path.abspath(sys.argv[sys.argv.index("--report") + 1])
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(report, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
