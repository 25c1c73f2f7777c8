"""Host side of ragged decode jobs (windows whose initial tokens differ in length in ONE lockstep job) on the CPU stand-in.

The stand-in (tests/oracle_engine.py) decodes window by window on the oracle, so a window's result cannot depend on the job
it is in: whatever differs between the ragged path and the grouped one (one job per distinct initial length) is host logic --
grouping, per-window ``sot_index``, slicing every window at its own ``sample_begin``.
"""
import os
import sys
import warnings
import zlib

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, HERE)

from oracle_engine import CpuWhisper, OracleEngine, install  # noqa: E402

BASE = dict(logprob_threshold=None, compression_ratio_threshold=None, no_speech_threshold=None, sample_len=24)


class RaggedOracleEngine(OracleEngine):
    """the stand-in with the product engine's ragged interface: init-token lists of any lengths, ``sot_index`` one value or one
    per window, ``sample_begin`` returned per window when they differ"""
    ragged_decode = True

    def __init__(self, oracle_model):
        super().__init__(oracle_model)
        self.jobs = []                # (temperature, initial lengths) of every decode call

    def decode(self, xkv, init_tokens, *, sot_index=0, ts_mask=None, window_uid=None, **kw):
        W = xkv.n_windows
        begins = [len(t) for t in init_tokens]
        sots = list(sot_index) if isinstance(sot_index, (list, tuple)) else [sot_index] * W
        self.jobs.append((kw.get("temperature", 0.0), tuple(begins)))
        parts = []
        for w in range(W):
            # the stand-in samples from torch's global generator; key the draws of a window on the window (its uid, its initial
            # tokens, its audio features, the temperature) like the device's counter-based hash, so that a sampled retry does not
            # depend on the job it is decoded in
            key = repr((None if window_uid is None else int(window_uid[w]), tuple(init_tokens[w]), kw.get("temperature", 0.0),
                        float(xkv.xa[w].double().sum())))
            torch.manual_seed(zlib.crc32(key.encode()))
            parts.append(OracleEngine.decode(self, xkv.select([w]), [init_tokens[w]], sot_index=sots[w],
                                             ts_mask=None if ts_mask is None else ts_mask[w:w + 1], **kw))
        self.n_decode_calls -= W - 1
        out = {k: np.concatenate([p[k] for p in parts]) for k in ("tokens", "lens", "sum_logprobs", "no_speech_prob")}
        uniform = len(set(begins)) == 1 and len(set(sots)) == 1
        out.update(steps=parts[0]["steps"], sample_begin=begins[0] if uniform else np.asarray(begins))
        return out


@pytest.fixture(scope="module")
def oracle_model():
    from oracle.whisper.model import build_model
    return build_model("tiny.en", seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5)


def test_results_slices_every_window_at_its_own_begin(oracle_model):
    from stable_ts_amd.decoding import DecodingOptions, DecodingPlan
    plan = DecodingPlan(CpuWhisper(oracle_model), DecodingOptions(language="en", beam_size=2))
    eot, TS = plan.tokenizer.eot, 449
    toks = np.full((2, 2, TS), eot, dtype=np.int32)
    toks[0, 0, :1], toks[0, 0, 1:4] = [plan.tokenizer.sot], [300, 301, 302]
    toks[0, 1, :1], toks[0, 1, 1:3] = [plan.tokenizer.sot], [400, 401]
    toks[1, 0, :7], toks[1, 0, 7:9] = [9] * 7, [500, 501]
    out = dict(tokens=toks, lens=np.array([[3, 2], [2, -1]]), sum_logprobs=np.array([[-3.0, -1.0], [-2.0, 0.0]], dtype=np.float32),
               no_speech_prob=np.array([0.25, 0.5], dtype=np.float32), steps=3, sample_begin=np.array([1, 7]))
    r = plan.results(out, [None, None], ["en", "en"])
    assert r[0].tokens == [400, 401] and r[1].tokens == [500, 501]          # window 0: -1 / 2 beats -3 / 3
    assert r[0].avg_logprob == pytest.approx(-1.0 / 3) and r[1].avg_logprob == pytest.approx(-2.0 / 3)
    assert r[1].no_speech_prob == 0.5
    # one common begin is still an int
    one = plan.results(dict(out, sample_begin=1), [None, None], ["en", "en"])
    assert one[0].tokens == [400, 401] and one[1].tokens == [9, 9]                 # (sliced at 1: two tokens of its prompt)


@pytest.mark.parametrize("ragged", [False, True])
def test_decode_windows_with_unequal_prompts(oracle_model, monkeypatch, ragged):
    """three windows, prompts of 0 / 3 / 6 tokens: on the unmodified stand-in (no ragged_decode: one job per length; this raised
    NotImplementedError) and on the ragged one (one job) -- every window equals the window decoded alone with its prompt"""
    from stable_ts_amd.decoding import DecodingOptions, decode_windows
    install(monkeypatch)
    model = CpuWhisper(oracle_model)
    if ragged:
        model.engine = RaggedOracleEngine(oracle_model)
    xa = model.encoder(0.1 * torch.randn(3, model.dims.n_mels, 3000, generator=torch.Generator().manual_seed(3)))
    xkv = model.cross_kv(xa)
    prompts = [None, [1000, 2000, 3000], [1000, 2000, 3000, 4000, 5000, 6000]]
    opts = DecodingOptions(language="en", sample_len=12, min_tokens=12, fp16=False)
    got = decode_windows(model, xkv, opts, prompts=prompts)
    assert model.engine.n_decode_calls == (1 if ragged else 3)
    for w in range(3):
        alone = decode_windows(model, xkv.select([w]), opts, prompts=[prompts[w]])[0]
        assert got[w].tokens == alone.tokens and len(alone.tokens) == 12
        assert got[w].avg_logprob == alone.avg_logprob and got[w].no_speech_prob == alone.no_speech_prob
    assert len({tuple(r.tokens) for r in got}) == 3


# transcribe_spans options of the span tests: everything at its default (condition_on_previous_text, the temperature ladder,
# compression_ratio_threshold 2.4, no_speech_threshold 0.6) except two.  logprob_threshold is off, because random weights score
# about -9 nats per token and can never meet -1.0: with it every window falls to temperature 1.0 and resets its prompt, and no two
# prompts ever differ.  sample_len 24 keeps the oracle affordable.
SPAN_OPTS = dict(language="en", sample_len=24, logprob_threshold=None)


def _rounds(jobs):
    """split the decode calls into lockstep rounds: a round starts at temperature 0 and walks UP the ladder"""
    out = []
    for t, b in jobs:
        if t == 0.0:
            out.append([])
        out[-1].append((t, b))
    return out


def test_transcribe_spans_ragged_equals_grouped(oracle_model, monkeypatch):
    """transcribe_spans over four spans of four to five windows (tiny.en, seed 1234, embed_gain 2.0, ts_gain 0.5: the golden cases'
    weights; make_golden.synth_audio(480 s, seed 31)), options SPAN_OPTS.  The greedy transcripts of some windows are repetitive
    enough to miss the compression-ratio threshold and are re-decoded at 0.2 / 0.4 while the others keep theirs, every span
    carries its own history, and so both the rounds' first jobs and the RETRIES of a pending subset hold several prompt lengths.
    The ragged engine gets one decode call per round and temperature; the result equals the grouped path's (same engine, switch
    off) segment for segment.  (The unmodified stand-in is not the grouped reference here: it samples from torch's global
    generator in call order, which regrouping changes; RaggedOracleEngine keys the draws on the window.)"""
    import make_golden as G
    import stable_ts_amd.decoding as D
    from stable_ts_amd.spans import transcribe_spans
    install(monkeypatch)
    audio = torch.as_tensor(G.synth_audio(480.0, seed=31))

    def run(switch):
        monkeypatch.setattr(D, "RAGGED_DECODE", switch)
        model = CpuWhisper(oracle_model)
        model.engine = RaggedOracleEngine(oracle_model)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            res = transcribe_spans(model, audio, 4, **SPAN_OPTS)
        return res.to_dict(), model.engine

    want, eng_off = run(False)
    got, eng = run(True)
    assert len(want["segments"]) > 8
    assert got == want
    assert all(len(set(b)) == 1 for _, b in eng_off.jobs)
    assert any(len(set(b)) > 1 for t, b in eng.jobs if t == 0.0), eng.jobs
    # a retry (t > 0) of a PENDING SUBSET that held two prompt lengths
    rounds = _rounds(eng.jobs)
    assert any(t > 0 and len(set(b)) > 1 and len(b) < len(r[0][1]) for r in rounds for t, b in r), eng.jobs
    # one call per (round, temperature): inside a round the temperatures strictly rise and the pending set only shrinks; the
    # grouped path has the same rounds and temperatures, with one call per distinct length
    for r in rounds:
        ts = [t for t, _ in r]
        assert ts == sorted(set(ts)) and all(len(b1) >= len(b2) for (_, b1), (_, b2) in zip(r, r[1:])), r
    keys_on = [(i, t) for i, r in enumerate(rounds) for t, _ in r]
    keys_off = [(i, t) for i, r in enumerate(_rounds_grouped(eng_off.jobs)) for t, _ in r]
    assert keys_on == sorted(set(keys_off))
    assert eng.n_decode_calls == len(keys_on) < eng_off.n_decode_calls


def _rounds_grouped(jobs):
    """the grouped path's calls: several per (round, temperature); a new round starts where the temperature falls back to 0"""
    out, last = [], None
    for t, b in jobs:
        if t == 0.0 and (last is None or last > 0.0 or not out):
            out.append([])
        out[-1].append((t, b))
        last = t
    return out
