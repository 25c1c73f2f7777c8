"""``locate_many`` on hardware: the device reduction of the greedy step (``swx_forward_next_token``) and the recordings in lockstep.

* ``swx_test_next_token_reduce`` (the reduction kernel alone, on scripted logits) against a numpy statement: ``np.lexsort`` on
  (index, logit) for the two best ids -- equal exactly -- and an f64 softmax for the three probabilities, |d log p| <= 5e-5 (the
  project's bar for f32 softmax arithmetic over a vocabulary-sized row; a probability the statement gives as exactly 0 must be
  exactly 0).  The padding behind column ``eot`` of every row is +inf, so a read past ``eot`` would show as a wrong arg-max.
* ``Engine.forward_next_token`` against ``forward_logits`` plus the host arithmetic of ``locator.next_token_on_host``: ids equal,
  probabilities within the same bar, every window alone the same BITS as in the batch; random weights with ``embed_gain=2.0``,
  tiny and base, f32 and f16, five windows of 1-30 tokens, two of them behind a prompt.  The seed of the token rows is one at
  which the host statement's three largest logits of every row lie more than 1e-3 apart (asserted).
* end to end with the golden case's sharp tiny.en weights on four synthetic recordings (33 s, 20 s, 47 s, and the 33-s tensor once
  more with another text), modes 0, 1 and 2, ``probability_threshold=0.0``.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
LOG_BAR = 5e-5
_CACHE = {}


def _synth_audio(seconds, seed):
    import importlib.util
    if "synth" not in _CACHE:
        spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "golden", "make_golden.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _CACHE["synth"] = mod.synth_audio
    return torch.as_tensor(_CACHE["synth"](seconds, seed), dtype=torch.float32)


# ------------------------------------------------------------------------------------------- the reduction kernel alone
def statement(rows, eot, suppress, targets):
    """numpy: ids by lexsort on (index, logit), probabilities by an f64 softmax over x[:eot]"""
    top, prob = [], []
    for row, target in zip(rows, targets):
        x = row[: eot + 1].astype(np.float32).copy()
        for v in suppress:
            if 0 <= v < eot:
                x[v] = -np.inf
        order = np.lexsort((np.arange(eot + 1), x))
        t0, t1 = int(order[-1]), int(order[-2])
        z = x[:eot].astype(np.float64)
        e = np.exp(z - z.max())
        p = e / e.sum()
        top.append((t0, t1))
        prob.append([float(p[i]) if 0 <= i < eot else 0.0 for i in (target, t0, t1)])
    return np.asarray(top), np.asarray(prob)


def reduce_on_device(rows, eot, suppress, targets):
    from stable_ts_amd import _lib
    from stable_ts_amd.engine import _ptr
    lib = _lib.load()
    W, ld = rows.shape
    d_rows = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    d_sup = torch.tensor(np.asarray(list(suppress) or [0], dtype=np.int32)).cuda()
    d_tgt = torch.tensor(np.asarray(targets, dtype=np.int32)).cuda()
    top = torch.full((W, 2), -7, dtype=torch.int32, device="cuda")
    prob = torch.full((W, 3), -7.0, dtype=torch.float32, device="cuda")
    _lib.check(lib.swx_test_next_token_reduce(_ptr(d_rows), ld, W, eot, _ptr(d_sup) if suppress else None, len(suppress), _ptr(d_tgt),
                                              _ptr(top), _ptr(prob), None), "swx_test_next_token_reduce")
    torch.cuda.synchronize()
    return top.cpu().numpy(), prob.cpu().numpy()


def close_in_log(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    zero = want == 0.0
    if not np.array_equal(got[zero], want[zero]) or np.any(got[~zero] <= 0.0):
        return False
    return bool(np.all(np.abs(np.log(got[~zero]) - np.log(want[~zero])) <= LOG_BAR))


def scripted(eot):
    """[(name, rows [3][ld], suppress list, targets [3])]; ld = eot + 6, columns past eot are +inf"""
    rng = np.random.default_rng(eot)
    ld = eot + 6

    def base():
        rows = (3.0 * rng.standard_normal((3, ld))).astype(np.float32)
        rows[:, eot + 1:] = np.inf
        return rows

    def pair(row, i, j):
        row[i] = row[j] = np.float32(row[: eot + 1].max() + 1.5)

    out = []
    # a tie of the two largest values: neighbouring lanes, different waves (or threads 256 apart), and eot - 1 / eot
    rows = base()
    pair(rows[0], 0, min(1, eot))
    pair(rows[1], min(5, eot), min(5 + 64, eot) if eot > 5 else 0)
    pair(rows[2], eot - 1, eot)
    out.append(("ties", rows, [], [-1, eot, eot - 1]))
    rows = base()
    pair(rows[0], min(3, eot - 1), min(3 + 256, eot))
    pair(rows[1], eot // 2, eot)
    rows[2, : eot + 1] = np.float32(0.25)                                  # every entry ties: eot, then eot - 1
    out.append(("ties_far", rows, [], [0, min(3, eot - 1), eot - 1]))
    # the arg-max suppressed / a suppressed target / the arg-max at eot; ids outside [0, eot) in the list are ignored
    rows = base()
    rows[2, eot] = np.float32(rows[2, : eot + 1].max() + 2.0)
    first = int(np.argmax(rows[0, :eot]))
    rows[0, first] = np.float32(rows[0, : eot + 1].max() + 1.0)
    inside = []
    for v in (first, int(np.argmax(rows[1, :eot])), eot // 3):
        if v not in inside and len(inside) + 1 < eot:                      # at least one id below eot stays
            inside.append(v)
    out.append(("suppressed", rows, [-5] + inside + [eot, eot + 3, 10 ** 6], [first, eot // 3, (eot // 3 + 1) % eot]))
    # everything below eot suppressed but one id
    rows = base()
    keep = eot // 2
    out.append(("all_but_one", rows, [v for v in range(eot) if v != keep], [keep, (keep + 1) % eot, -1]))
    return out


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("eot", [1, 2, 63, 64, 65, 255, 257, 1025, 50256])
def test_next_token_reduce_matches_the_numpy_statement(eot, W):
    for name, rows, suppress, targets in scripted(eot):
        want_top, want_prob = statement(rows, eot, suppress, targets)
        for w0 in range(0, 3, W):
            top, prob = reduce_on_device(rows[w0: w0 + W], eot, suppress, targets[w0: w0 + W])
            where = (name, eot, W, w0)
            assert np.array_equal(top, want_top[w0: w0 + W]), (where, top.tolist(), want_top[w0: w0 + W].tolist())
            assert close_in_log(prob, want_prob[w0: w0 + W]), (where, prob.tolist(), want_prob[w0: w0 + W].tolist())
        if name == "suppressed" and eot >= 63:
            assert want_top[0][0] != targets[0] and want_prob[0][0] == 0.0          # the raw arg-max is gone, its probability 0
            assert want_prob[1][0] == 0.0                                           # a suppressed target
            assert want_top[2][0] == eot and want_prob[2][1] == 0.0 and want_prob[2][2] > 0.0
        if name == "ties":
            assert tuple(want_top[2]) == (eot, eot - 1)


def test_next_token_reduce_refuses_bad_arguments():
    from stable_ts_amd import _lib
    from stable_ts_amd.engine import _ptr
    lib = _lib.load()
    x = torch.zeros(2, 16, device="cuda")
    t = torch.zeros(2, dtype=torch.int32, device="cuda")
    top = torch.zeros(2, 2, dtype=torch.int32, device="cuda")
    prob = torch.zeros(2, 3, device="cuda")
    call = lib.swx_test_next_token_reduce
    assert call(None, 16, 2, 8, None, 0, _ptr(t), _ptr(top), _ptr(prob), None) == -1
    assert call(_ptr(x), 16, 2, 0, None, 0, _ptr(t), _ptr(top), _ptr(prob), None) == -1           # eot <= 0
    assert call(_ptr(x), 16, 2, 16, None, 0, _ptr(t), _ptr(top), _ptr(prob), None) == -1          # ld <= eot
    assert call(_ptr(x), 16, 2, 8, None, 3, _ptr(t), _ptr(top), _ptr(prob), None) == -1           # a list without a pointer
    assert call(_ptr(x), 16, 2, 8, None, 0, _ptr(t), _ptr(top), _ptr(prob), None) == 0


# ------------------------------------------------------------------------------------------- the engine call
SEED = 3          # of the token rows below; the precondition on the logit gaps is asserted, not assumed


def _random_model(name, dtype):
    import stable_ts_amd as sw
    if (name, dtype) not in _CACHE:
        dims = sw.dims_for(name)
        m = sw.Whisper(dims, dtype=dtype, max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE[(name, dtype)] = m
    return _CACHE[(name, dtype)]


def _windows(model):
    from stable_ts_amd.tokenizer import get_tokenizer
    tok = get_tokenizer(True, num_languages=model.num_languages, language="en", task="transcribe")
    rng = np.random.default_rng(SEED)
    text = lambda n: [int(t) for t in rng.integers(300, 20000, n)]      # noqa: E731
    head = [*tok.sot_sequence, tok.no_timestamps]
    tokens = [[tok.sot], head[:2], head + text(3), [tok.sot_prev] + text(9) + head + text(16), [tok.sot_prev] + text(4) + head + text(7)]
    assert [len(t) for t in tokens] == [1, 2, 7, 30, 16]
    suppress = sorted(set(text(60) + [1, 2, 7, tok.eot - 1])) + [-3, tok.eot, tok.eot + 5]
    targets = [tokens[2][-1], -1, suppress[5], 1234, tok.eot]
    return tok, tokens, suppress, targets


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_forward_next_token_matches_forward_logits_and_host_arithmetic(name, dtype):
    from stable_ts_amd.locator import next_token_on_host
    from stable_ts_amd.transcribe import _xkv_select
    model = _random_model(name, dtype)
    eng = model.engine
    assert eng.device_next_token
    tok, tokens, suppress, targets = _windows(model)
    mel = model.log_mel_segments([_synth_audio(5.0, 50 + w)[:48000].cuda() for w in range(5)])
    xkv = model.cross_kv(model.encoder(mel))
    logits = eng.forward_logits(xkv, tokens)
    assert tuple(logits.shape) == (5, 30, model.dims.n_vocab)
    inside = [s for s in suppress if 0 <= s < tok.eot]
    want = []
    for w, t in enumerate(tokens):
        row = logits[w, len(t) - 1, : tok.eot + 1].float().cpu().clone()
        ans = next_token_on_host(row.clone(), tok.eot, inside, targets[w] if 0 <= targets[w] < tok.eot else -1)
        row[inside] = -np.inf
        best3 = row.sort().values[-3:]
        gaps = (best3[1:] - best3[:-1]).tolist()
        print(f"[next_token {name} {dtype}] window {w}: best {ans[0]}, runner-up {ans[1]}, gaps of the three largest logits {gaps}")
        assert min(gaps) > 1e-3, (w, gaps)                  # the precondition of an exact id comparison
        want.append(ans)
    top, prob = eng.forward_next_token(xkv, tokens, tok.eot, suppress, targets)
    assert top.dtype == np.int32 and prob.dtype == np.float32 and top.shape == (5, 2) and prob.shape == (5, 3)
    assert [(int(a), int(b)) for a, b in top] == [(a[0], a[1]) for a in want]
    assert close_in_log(prob, [[a[2], a[3], a[4]] for a in want]), (prob.tolist(), want)
    assert prob[1][0] == 0.0 and prob[2][0] == 0.0 and prob[4][0] == 0.0        # target -1, a suppressed target, target == eot
    for w in range(5):                                                          # a window alone: the same bits
        one_top, one_prob = eng.forward_next_token(_xkv_select(model, xkv, [w]), [tokens[w]], tok.eot, suppress, [targets[w]])
        assert np.array_equal(one_top[0], top[w]), w
        assert np.array_equal(one_prob[0].view(np.int32), prob[w].view(np.int32)), (w, one_prob[0].tolist(), prob[w].tolist())


def test_forward_next_token_refuses_bad_arguments():
    model = _random_model("tiny", "f16")
    eng = model.engine
    mel = model.log_mel_segments([_synth_audio(5.0, 1)[:16000].cuda()])
    xkv = model.cross_kv(model.encoder(mel))
    for eot in (0, model.dims.n_vocab):
        with pytest.raises(ValueError):
            eng.forward_next_token(xkv, [[1, 2]], eot, [], [-1])
    with pytest.raises(ValueError):
        eng.forward_next_token(xkv, [[1, 2]], 50257, [], [-1, 3])
    from stable_ts_amd.engine import _i32arr, _ptr
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    n_vocab = model.dims.n_vocab
    for eot, tokens in ((0, t), (n_vocab, t), (50257, None)):
        assert eng.lib.swx_forward_next_token(eng.h, _ptr(tokens), _i32arr([2]), 1, 2, eot, None, 0, _ptr(t), _ptr(xkv), _ptr(t),
                                              _ptr(t), eng.stream) == -1


def test_dtw_counts_beyond_the_matrix_mean_its_extent():
    """mode 0 asks for the word times of up to 33 s of a 30-s chunk (1650 frames of a 1500-frame matrix): the reference's slice
    stops at the matrix, and so does ``dtw`` -- the counts are clamped before they reach the kernel"""
    from stable_ts_amd.engine import dtw
    x = torch.randn(2, 12, 1500, generator=torch.Generator().manual_seed(5)).cuda()
    want = dtw(x, [9, 12], [1500, 1500])
    got = dtw(x, [9, 40], [1608, 1500])
    for (gi, gj), (wi, wj) in zip(got, want):
        assert np.array_equal(gi, wi) and np.array_equal(gj, wj) and gj.max() == 1499


# ------------------------------------------------------------------------------------------- end to end
TEXTS = [" aaat", " aabc aaat", [25, 31], " aabc"]
MODES = {0: dict(mode=0, count=2), 1: dict(mode=1, count=2), 2: dict(mode=2, count=0)}


def _sharp(dtype):
    import stable_ts_amd as sw
    if ("sharp", dtype) not in _CACHE:
        dims = sw.dims_for("tiny.en")
        m = sw.Whisper(dims, dtype=dtype, max_windows=1, max_rows=5)
        m.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        _CACHE[("sharp", dtype)] = m
    return _CACHE[("sharp", dtype)]


def _recordings():
    if "clips" not in _CACHE:
        a = _synth_audio(33.0, 61).cuda()
        _CACHE["clips"] = [a, _synth_audio(20.0, 62), _synth_audio(47.0, 63).cuda(), a]
    return _CACHE["clips"]


def _flat(matches):
    """[(what, tokens / words, times, probabilities)] per match"""
    out = []
    for x in matches:
        if isinstance(x, dict) and "target_end" in x:
            out.append(("end", [], [x["target_end"]], []))
        elif isinstance(x, dict):
            ws = x["duration_window_word"]
            out.append(("window", [(w["word"], tuple(w["tokens"])) for w in ws] + [x["text"], x["duration_window_text"]], [x["end"]],
                        [w["probability"] for w in ws]))
        else:
            out.append(("segment", [(w.word, tuple(w.tokens)) for w in x.words], [x.seek] + [t for w in x.words for t in (w.start, w.end)],
                        [float(w.probability) for w in x.words]))
    return out


def _loop(dtype, mode):
    """model.locate per recording (the parent commit's path), once per (dtype, mode): results and encoder passes per recording"""
    if ("loop", dtype, mode) not in _CACHE:
        model, res, calls = _sharp(dtype), [], []
        for a, t in zip(_recordings(), TEXTS):
            c0 = model.engine.encode_calls
            res.append(_flat(model.locate(a, t, "en", probability_threshold=0.0, verbose=None, **MODES[mode])))
            calls.append(model.engine.encode_calls - c0)
        _CACHE[("loop", dtype, mode)] = (res, calls)
    return _CACHE[("loop", dtype, mode)]


def _same(got, want, *, exact, time_bar=0.0):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert [(m[0], m[1]) for m in g] == [(m[0], m[1]) for m in w], i          # the matches, their words and tokens
        for mg, mw in zip(g, w):
            if time_bar:
                assert all(abs(a - b) <= time_bar + 1e-9 for a, b in zip(mg[2], mw[2])), (i, mg[2], mw[2])
            else:
                assert mg[2] == mw[2], (i, mg[2], mw[2])
            if exact:
                assert mg[3] == mw[3], (i, mg[3], mw[3])
            elif not time_bar:
                assert close_in_log(mg[3], mw[3]), (i, mg[3], mw[3])


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_locate_many_equals_locate_per_recording(dtype, mode):
    model = _sharp(dtype)
    want, calls = _loop(dtype, mode)
    assert all(len(w) > 0 for w in want) and (mode == 2 or all(m[1] for w in want for m in w))
    for probe in (False, True):
        c0, w0, bound0 = model.engine.encode_calls, model.engine.encode_windows, model.engine.max_windows
        got = [_flat(r) for r in model.locate_many(_recordings(), TEXTS, "en", max_tracks=4, device_probe=probe,
                                                   probability_threshold=0.0, verbose=None, **MODES[mode])]
        passes, windows = model.engine.encode_calls - c0, model.engine.encode_windows - w0
        print(f"[locate_many {dtype} mode {mode} device_probe={probe}] encoder passes {passes} for {windows} windows; the loop: {calls}")
        if dtype == "f32":
            _same(got, want, exact=not probe)
        else:
            _same(got, want, exact=False, time_bar=0.02)
        assert windows == sum(calls) and passes <= max(calls) < sum(calls)
        assert model.engine.max_windows <= max(bound0, 4)                        # the workspace grows to max_tracks windows


def test_locate_many_small_batches_and_default_probe():
    """max_tracks below the number of recordings (slots are handed on), and the default of ``device_probe``"""
    model = _sharp("f32")
    want, _ = _loop("f32", 1)
    got = [_flat(r) for r in model.locate_many(_recordings(), TEXTS, ["en"] * 4, max_tracks=3, device_probe=False,
                                               probability_threshold=0.0, verbose=None, **MODES[1])]
    _same(got, want, exact=True)
    got = [_flat(r) for r in model.locate_many(_recordings(), TEXTS, "en", max_tracks=2, probability_threshold=0.0, verbose=None,
                                               **MODES[1])]
    _same(got, want, exact=False)


def test_target_id_outside_the_text_vocabulary_raises_what_locate_raises():
    """a phrase token at or above ``eot`` is an IndexError in ``locate`` (the probability lookup); the kernel would answer 0 for it,
    so such a step is answered on the host and ``locate_many`` raises the same, whatever ``device_probe`` says"""
    model = _sharp("f32")
    clip = _recordings()[1]
    eot = 50256                                                              # tiny.en
    kw = dict(mode=1, probability_threshold=0.0, verbose=None)
    with pytest.raises(IndexError):
        model.locate(clip, [25, eot + 5], "en", **kw)
    for probe in (True, False):
        with pytest.raises(IndexError):
            model.locate_many([clip, clip], [[25, 31], [25, eot + 5]], "en", device_probe=probe, **kw)
