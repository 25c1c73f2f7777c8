"""Ragged decode jobs on the device: W windows whose initial tokens differ in length (and whose <|startoftranscript|> sits at
different indices) advance in ONE lockstep job (swx_decode_cfg.sample_begins / sot_indices).

The bar is the project's batch invariance (tests/test_gpu_batch_invariance.py): every window of the ragged job equals the same
window decoded alone -- tokens, lengths, sums of log-probabilities, no-speech probability, np.array_equal.  Models and helpers
as in tests/test_gpu_model.py: tiny.en / base.en architecture, seeded random weights, both dtypes.
"""
import numpy as np
import pytest
import torch

from oracle import stable as ost
from oracle.whisper import model as om
from oracle.whisper.decoding import DecodingOptions

pytestmark = pytest.mark.gpu

_CACHE = {}
KEYS = ("tokens", "lens", "sum_logprobs", "no_speech_prob")


def _oracle(name, gain=3.0):
    if ("o", name, gain) not in _CACHE:
        _CACHE[("o", name, gain)] = om.build_model(name, seed=1234, std=0.02, embed_gain=gain)
    return _CACHE[("o", name, gain)]


def _engine(name, dtype, gain=3.0):
    from stable_ts_amd.engine import Engine, ModelDimensions
    if ("e", name, dtype, gain) not in _CACHE:
        d = om.dims_for(name)
        eng = Engine(ModelDimensions(**d.__dict__), dtype=dtype, max_windows=7, max_rows=35)
        eng.load_state_dict(om.random_state_dict(d, 1234, 0.02, gain))
        _CACHE[("e", name, dtype, gain)] = eng
    return _CACHE[("e", name, dtype, gain)]


def _mel(n_mels, seed, B):
    g = torch.Generator().manual_seed(seed)
    t = torch.linspace(0, 1, 3000)
    base = torch.sin(t[None, None, :] * (5 + torch.arange(n_mels)[None, :, None] * 0.37)) * 0.5
    return (base + 0.3 * torch.randn(B, n_mels, 3000, generator=g)).float()


def _tok_cfg(task):
    tok = task.tokenizer
    return dict(eot=tok.eot, sot=tok.sot, no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin,
                no_speech=tok.no_speech, blank_token=tok.encode(" ")[0], suppress_tokens=list(task._get_suppress_tokens()))


def _inits(tok, lengths, seed=5):
    """raw initial-token lists: [sot] for length 1, else [sot_prev, <text ids>, sot] (the shape transcribe() carries over);
    and the index of sot in each"""
    rng = np.random.RandomState(seed)
    inits = []
    for n in lengths:
        inits.append([tok.sot] if n == 1 else [tok.sot_prev] + [int(t) for t in rng.randint(300, 20000, size=n - 2)] + [tok.sot])
    return inits, [len(t) - 1 for t in inits]


LENGTHS = (1, 5, 12, 18, 151, 228, 1)

MODES = {
    "greedy": dict(n_group=1, beam=False),
    "beam5": dict(n_group=5, beam=True),
    "sample": dict(n_group=3, beam=False, temperature=0.7, seed=11),
}


def _xkvs(eng, mels):
    """cross-K/V of the batch and of every window alone (the encoder is batch invariant: test_gpu_batch_invariance)"""
    both = eng.cross_kv(eng.encode(mels.cuda().contiguous()))
    return both, [eng.cross_kv(eng.encode(mels[w:w + 1].cuda().contiguous())) for w in range(mels.shape[0])]


def _assert_window_equal(job, w, one, what):
    for k in KEYS:
        a, b = np.asarray(job[k][w]), np.asarray(one[k][0])
        assert np.array_equal(a, b, equal_nan=True), (what, w, k, a, b)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,dtype", [("tiny.en", "f16"), ("tiny.en", "f32"), ("base.en", "f16"), ("base.en", "f32")])
def test_ragged_job_equals_the_windows_alone(name, dtype, mode):
    """1: seven windows, 1 / 5 / 12 / 18 / 151 / 228 / 1 initial tokens, each with its own sot_index, one job vs window by window.
    5 next to 12 share a padded prefill run on both sides of the self-attention's 8-token threshold, 18 next to 228 on both sides
    of its 32-token one; 1 next to 228 puts a short window under the long step-attention variant; the second single-token window
    makes one more prefill run"""
    m, eng = _oracle(name), _engine(name, dtype)
    task = ost.DecodingTaskStable(m, DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, sample_len=24))
    inits, sots = _inits(task.tokenizer, LENGTHS)
    uids = [7, 1500, 3000, 42, 9000, 11, 4500]
    kw = dict(sample_len=24, min_tokens=10, **MODES[mode], **_tok_cfg(task))
    both, alone = _xkvs(eng, _mel(m.dims.n_mels, 77, len(LENGTHS)))
    job = eng.decode(both, inits, sot_index=sots, window_uid=uids, **kw)
    assert list(job["sample_begin"]) == list(LENGTHS)
    for w in range(len(LENGTHS)):
        one = eng.decode(alone[w], [inits[w]], sot_index=sots[w], window_uid=[uids[w]], **kw)
        assert one["sample_begin"] == len(inits[w])
        _assert_window_equal(job, w, one, (name, dtype, mode))
        sb = len(inits[w])
        assert job["tokens"][w, 0, :sb].tolist() == inits[w]
        assert int(job["lens"][w].max()) >= 10


@pytest.mark.parametrize("mode", ["greedy", "beam5"])
@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_context_full_is_per_window(dtype, mode):
    """2: n_text_ctx - 9 initial tokens next to a short prompt, budget 20, EOT suppressed: the long window leaves the loop after
    10 samples (tokens.shape[-1] > n_ctx, decode.py:60), the short one after 20; both as alone"""
    name = "tiny.en"
    m, eng = _oracle(name), _engine(name, dtype)
    task = ost.DecodingTaskStable(m, DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, sample_len=20))
    n_ctx = m.dims.n_text_ctx
    inits, sots = _inits(task.tokenizer, (n_ctx - 9, 6, n_ctx - 9), seed=8)
    kw = dict(sample_len=20, min_tokens=20, **MODES[mode], **_tok_cfg(task))
    both, alone = _xkvs(eng, _mel(m.dims.n_mels, 78, 3))
    job = eng.decode(both, inits, sot_index=sots, **kw)
    assert job["steps"] == 20
    for w in range(3):
        one = eng.decode(alone[w], [inits[w]], sot_index=sots[w], **kw)
        _assert_window_equal(job, w, one, (dtype, mode))
        want = 10 if w != 1 else 20
        assert one["steps"] == want
        assert [int(x) for x in job["lens"][w] if x >= 0] == [want] * task_n(job, w), job["lens"][w]


def task_n(job, w):
    return int((np.asarray(job["lens"][w]) >= 0).sum())


def _cfg_with_arrays(begins, sots):
    """a swx_decode_cfg factory that always passes the per-window arrays through the C ABI (Engine.decode itself folds entries
    that all agree to NULL)"""
    import ctypes
    from stable_ts_amd._lib import swx_decode_cfg

    def make(**kw):
        kw["sample_begins"] = (ctypes.c_int32 * len(begins))(*begins)
        kw["sot_indices"] = (ctypes.c_int32 * len(sots))(*sots)
        return swx_decode_cfg(**kw)
    return make


@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_uniform_jobs_are_untouched(mode, monkeypatch):
    """3: one common length given as NULL arrays and as arrays whose entries all agree: the same results, both from the replayed
    step graph, the second from the graph the first captured"""
    import stable_ts_amd.engine as E
    name = "tiny.en"
    m, eng = _oracle(name), _engine(name, "f16")
    task = ost.DecodingTaskStable(m, DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, sample_len=24,
                                                     prompt=list(range(1000, 1012))))
    init = list(task.initial_tokens)
    kw = dict(sample_len=24, min_tokens=24, sot_index=task.sot_index, **MODES[mode], **_tok_cfg(task))
    both, _ = _xkvs(eng, _mel(m.dims.n_mels, 79, 3))
    st0 = eng.graph_stats()
    a = eng.decode(both, [init] * 3, **kw)
    st1 = eng.graph_stats()
    assert not st1["fell_back"], st1
    monkeypatch.setattr(E, "swx_decode_cfg", _cfg_with_arrays([len(init)] * 3, [task.sot_index] * 3))
    b = eng.decode(both, [init] * 3, **kw)
    st2 = eng.graph_stats()
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["steps"] == b["steps"] == 24
    assert not st2["fell_back"], st2
    assert st1["replays"] - st0["replays"] >= 10 and st2["replays"] - st1["replays"] >= 10, (st0, st1, st2)
    assert st2["captures"] == st1["captures"], (st1, st2)            # the same graph key: no new capture


@pytest.mark.parametrize("mode", list(MODES))
def test_ragged_graph_replay_is_bit_identical(mode):
    """4: the captured two-step graph on a ragged job vs every step launched eagerly (SWX_FLAG_NO_GRAPH = 16384)"""
    from stable_ts_amd import _lib
    lib = _lib.load()
    name = "base.en"
    m, eng = _oracle(name), _engine(name, "f16")
    task = ost.DecodingTaskStable(m, DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, sample_len=30))
    n_ctx = m.dims.n_text_ctx
    inits, sots = _inits(task.tokenizer, (1, 40, n_ctx - 14, 200), seed=2)
    kw = dict(sample_len=30, min_tokens=6, window_uid=[1, 2, 3, 4], **MODES[mode], **_tok_cfg(task))
    both, _ = _xkvs(eng, _mel(m.dims.n_mels, 80, 4))
    old = lib.swx_debug_flags(-1)
    st0 = eng.graph_stats()
    try:
        assert not (old & 16384)
        g = eng.decode(both, inits, sot_index=sots, **kw)
        st1 = eng.graph_stats()
        lib.swx_debug_flags(old | 16384)
        e = eng.decode(both, inits, sot_index=sots, **kw)
    finally:
        lib.swx_debug_flags(old)
    for k in KEYS:
        assert np.array_equal(g[k], e[k], equal_nan=True), k
    assert g["steps"] == e["steps"]
    assert not st1["fell_back"] and st1["replays"] - st0["replays"] >= (int(g["steps"]) - 4) // 2, (st0, st1, g["steps"])


def _rank(out, w):
    scores = []
    for k in range(out["tokens"].shape[1]):
        ln = int(out["lens"][w, k])
        scores.append(-np.inf if ln <= 0 else out["sum_logprobs"][w, k] / ln)
    return int(np.argmax(scores))


@pytest.mark.parametrize("beam", [False, True])
def test_ragged_strict_f32_against_the_oracle(beam):
    """5: one ragged job with prompts vs oracle.stable.DecodingTaskStable window by window: identical tokens, avg_logprob
    within 1e-3 (the bounds of test_gpu_model.py::test_decode_strict_f32_identical_tokens)"""
    name = "tiny.en"
    m, eng = _oracle(name), _engine(name, "f32")
    mels = _mel(m.dims.n_mels, 21, B=3)
    prompts = [None, [1000, 2000, 3001, 40000, 7], [int(t) for t in np.random.RandomState(4).randint(300, 20000, size=60)]]
    o = dict(sample_len=24, beam_size=5 if beam else None)
    tasks, want = [], []
    for w in range(3):
        options = DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, prompt=prompts[w], **o)
        tasks.append(ost.DecodingTaskStable(m, options))
        want.append(ost.decode_stable(m, mels[w], options, min_tokens=24)[0])
    both, _ = _xkvs(eng, mels)
    out = eng.decode(both, [list(t.initial_tokens) for t in tasks], sot_index=[t.sot_index for t in tasks],
                     n_group=tasks[0].n_group, beam=beam, sample_len=24, min_tokens=24, **_tok_cfg(tasks[0]))
    assert len(set(out["sample_begin"])) == 3
    for w in range(3):
        sb, best = int(out["sample_begin"][w]), _rank(out, w)
        got = out["tokens"][w, best, sb: sb + int(out["lens"][w, best])].tolist()
        assert got == want[w].tokens, (w, got, want[w].tokens)
        assert abs(out["sum_logprobs"][w, best] / (len(got) + 1) - want[w].avg_logprob) < 1e-3
        assert abs(out["no_speech_prob"][w] - want[w].no_speech_prob) < 1e-4 + 1e-2 * want[w].no_speech_prob


def test_bad_per_window_arguments_are_rejected():
    from stable_ts_amd._lib import SwxError
    name = "tiny.en"
    m, eng = _oracle(name), _engine(name, "f16")
    task = ost.DecodingTaskStable(m, DecodingOptions(fp16=False, language="en", max_initial_timestamp=None, sample_len=4))
    inits, sots = _inits(task.tokenizer, (1, 9))
    both, _ = _xkvs(eng, _mel(m.dims.n_mels, 81, 2))
    kw = dict(sample_len=4, **_tok_cfg(task))
    with pytest.raises(SwxError, match="invalid argument"):
        eng.decode(both, inits, sot_index=[0, 9], **kw)                    # outside the window's initial tokens
    with pytest.raises(SwxError, match="invalid argument"):
        eng.decode(both, [inits[0], [task.tokenizer.sot] * (m.dims.n_text_ctx + 1)], sot_index=[0, 0], **kw)
    eng.decode(both, inits, sot_index=sots, **kw)                          # the handle is fine afterwards


def test_transcribe_spans_one_job_per_round():
    """6: transcribe_spans over four spans of four to five windows, strict f32, the golden cases' weights (tiny.en, seed 1234,
    embed_gain 2.0, ts_gain 0.5), make_golden.synth_audio(480 s, seed 31).  Options: the defaults (condition_on_previous_text,
    the temperature ladder, compression_ratio_threshold 2.4, no_speech_threshold 0.6) except logprob_threshold=None -- random
    weights score about -9 nats per token and can never meet -1.0, so with it every window falls to temperature 1.0, resets its
    prompt, and no two prompts ever differ -- and sample_len=24 as in the CPU twin of this test.  The greedy transcripts of some
    windows miss the compression-ratio threshold and are re-decoded (sampled, keyed on window_uid) while the others keep theirs,
    and every span carries its own history.  Same to_dict() with the switch on and off; one decode call per round and temperature
    with it on, fewer than with it off; at least one round's first job AND at least one retry of a pending subset (t > 0, through
    _xkv_select) held two prompt lengths."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    import stable_ts_amd as sw
    import stable_ts_amd.decoding as D
    dims = sw.dims_for("tiny.en")
    model = sw.Whisper(dims, dtype="f32", max_windows=4, max_rows=20)
    model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
    audio = torch.as_tensor(G.synth_audio(480.0, seed=31))
    kw = dict(language="en", sample_len=24, logprob_threshold=None)
    jobs = []
    real = model.engine.decode

    def counted(xkv, init_tokens, **k):
        jobs[-1].append((float(k.get("temperature", 0.0)), tuple(len(t) for t in init_tokens), xkv.n_windows))
        return real(xkv, init_tokens, **k)

    model.engine.decode = counted
    outs = {}
    old = D.RAGGED_DECODE
    try:
        for switch in (False, True):
            D.RAGGED_DECODE = switch
            jobs.append([])
            outs[switch] = model.transcribe_spans(audio, 4, **kw).to_dict()
    finally:
        D.RAGGED_DECODE = old
    grouped, ragged = jobs
    print("ragged jobs:", ragged)
    assert outs[True] == outs[False] and len(outs[True]["segments"]) > 8
    assert all(len(set(b)) == 1 for _, b, _ in grouped), grouped
    assert all(n == len(b) for _, b, n in ragged)
    rounds = []
    for t, b, _ in ragged:
        if t == 0.0:
            rounds.append([])
        rounds[-1].append((t, b))
    for r in rounds:                       # one call per (round, temperature); the pending set only shrinks
        ts = [t for t, _ in r]
        assert ts == sorted(set(ts)) and all(len(b1) >= len(b2) for (_, b1), (_, b2) in zip(r, r[1:])), r
    assert any(len(set(b)) > 1 for r in rounds for t, b in r if t == 0.0), ragged
    assert any(t > 0 and len(set(b)) > 1 and len(b) < len(r[0][1]) for r in rounds for t, b in r), ragged
    assert len(ragged) < len(grouped), (len(ragged), len(grouped))
