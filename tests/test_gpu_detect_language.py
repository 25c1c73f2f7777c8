"""``Engine.detect_language`` (``swx_detect_language``) on hardware: the language of windows whose cross-K/V is resident, from
one decoder step at <|startoftranscript|> and the language rows of the embedding, against the unchanged host path
``Whisper.detect_language`` (vocabulary-wide projection, ``[W, n_vocab]`` f32 to the host, mask + softmax there) on the same
encoder features.

Models (seeded random weights, the recipe of tests/test_gpu_golden.py: seed 1234, std 0.02, embed_gain 2.0, ts_gain 0.5):
  * ``tiny``  -- multilingual tiny, n_vocab 51 865, 99 languages, n_text_state 384 (a 16-byte f16 load per lane leaves 16 lanes
    of a wave idle);
  * ``wide2`` -- n_vocab 51 866, 100 languages, 2 + 2 layers, n_text_state 1280, 128 mels: the widest row, and a language count
    that neither the 4 waves nor the 256 threads of the workgroup divide.
Audio: 30 s of seeded noise + a gated tone (``_audio``), seeds 11 / 12 / 13.

Near ties: the comparison tolerates 5e-5 (f32) / 1e-3 (f16) in log p, so the inputs were chosen with the top two languages
further apart than that by a wide margin.  On the CPU oracle (oracle.whisper.decoding.detect_language, f32) the gaps in log p
between the best and the second language are
    tiny   seeds 11 / 12 / 13:  0.7916 / 0.7912 / 0.7929   (best: be, p = 0.070; smallest p of any language 2.1e-3)
    wide2  seeds 11 / 12 / 13:  0.1221 / 0.1461 / 0.1899   (best: hi, p = 0.137; smallest p of any language 1.0e-4)
and the tests assert ``>= 1e-2`` on the host path's numbers again, so a near tie cannot hide behind the tolerance.  Every language
has p >= 1e-6 with these inputs: the comparison runs over all of them.  Observed max |delta log p| on hardware: tiny 1.1e-6 (f32) /
5.7e-7 (f16), wide2 6.1e-6 (f32) / 1.5e-6 (f16).
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)
# |delta log p|: the project's strict per-token bound (f32) and its fp16 log-prob bound (README, Parity)
TOL = {"f32": 5e-5, "f16": 1e-3}
_CACHE = {}


def _dims(name):
    import stable_ts_amd as sw
    if name == "tiny":
        return sw.dims_for("tiny")
    return sw.ModelDimensions(128, 1500, 1280, 20, 2, 51866, 448, 1280, 20, 2)


def _audio(seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(480000) / 16000.0
    f = 120.0 + 40.0 * (seed % 7)
    return (0.05 * torch.randn(480000, generator=g) + 0.1 * torch.sin(2 * np.pi * f * t) * (torch.sin(2 * np.pi * 1.5 * t) > 0)).float()


def _setup(name, dtype):
    """model, its tokenizer, the encoder features of the three windows, and the host path's answer on them (computed once)"""
    import stable_ts_amd as sw
    from stable_ts_amd.tokenizer import get_tokenizer
    key = (name, dtype)
    if key not in _CACHE:
        dims = _dims(name)
        model = sw.Whisper(dims, dtype=dtype, max_windows=3, max_rows=5)
        model.load_state_dict(sw.random_state_dict(dims, seed=1234, std=0.02, embed_gain=2.0, ts_gain=0.5))
        tok = get_tokenizer(True, num_languages=model.num_languages)
        mel = model.log_mel_batch([_audio(s) for s in SEEDS], [0] * len(SEEDS))
        feats = model.encoder(mel)
        host_tok, host_probs = model.detect_language(feats)
        _CACHE[key] = model, tok, feats, [int(t) for t in host_tok], host_probs
    return _CACHE[key]


CASES = [("tiny", "f32"), ("tiny", "f16"), ("wide2", "f32"), ("wide2", "f16")]


@pytest.mark.parametrize("W", [1, 3])
@pytest.mark.parametrize("name,dtype", CASES)
def test_device_language_equals_host_path(name, dtype, W):
    model, tok, feats, host_tok, host_probs = _setup(name, dtype)
    lang_tokens = list(tok.all_language_tokens)
    assert len(lang_tokens) == (99 if name == "tiny" else 100) and model.engine.device_language_id
    best, probs = model.engine.detect_language(model.cross_kv(feats[:W]), tok.sot, lang_tokens)
    assert best.shape == (W,) and probs.shape == (W, len(lang_tokens)) and probs.dtype == np.float32
    for w in range(W):
        hp = np.array([host_probs[w][c] for c in tok.all_language_codes], dtype=np.float64)
        top2 = np.sort(np.log(hp))[-2:]
        assert top2[1] - top2[0] >= 1e-2, "input condition: the top two languages must not be a near tie"
        assert int(best[w]) == host_tok[w] == lang_tokens[int(np.argmax(probs[w]))]
        sel = hp >= 1e-6
        assert sel.sum() >= 2
        err = np.abs(np.log(probs[w].astype(np.float64)[sel]) - np.log(hp[sel])).max()
        print(f"{name} {dtype} W={W} w={w}: max |dlogp| = {err:.3e}, sum = {probs[w].astype(np.float64).sum():.8f}")
        assert err <= TOL[dtype], (name, dtype, W, w, err)
        assert abs(probs[w].astype(np.float64).sum() - 1.0) <= 1e-5


@pytest.mark.parametrize("name,dtype", CASES)
def test_window_of_a_batch_is_the_window_alone(name, dtype):
    """window k of the W = 3 call against the same window in a W = 1 call: bit-identical probabilities, the same token"""
    model, tok, feats, _, _ = _setup(name, dtype)
    lang_tokens = list(tok.all_language_tokens)
    best3, probs3 = model.engine.detect_language(model.cross_kv(feats), tok.sot, lang_tokens)
    for w in range(3):
        best1, probs1 = model.engine.detect_language(model.cross_kv(feats[w:w + 1]), tok.sot, lang_tokens)
        assert best1[0] == best3[w]
        assert np.array_equal(probs1[0].view(np.uint32), probs3[w].view(np.uint32)), (name, dtype, w)


def test_ties_go_to_the_lowest_index_and_order_follows_the_list():
    """the same token listed twice ties exactly: the first entry wins (torch.argmax); a permuted list permutes the output"""
    model, tok, feats, host_tok, _ = _setup("tiny", "f32")
    lang_tokens = list(tok.all_language_tokens)
    xkv = model.cross_kv(feats[:1])
    _, ref = model.engine.detect_language(xkv, tok.sot, lang_tokens)
    top = host_tok[0]
    best, probs = model.engine.detect_language(xkv, tok.sot, [lang_tokens[0], top, lang_tokens[1], top])
    assert int(best[0]) == top and probs[0, 1] == probs[0, 3] and int(np.argmax(probs[0])) == 1
    rev = lang_tokens[::-1]
    best_r, probs_r = model.engine.detect_language(xkv, tok.sot, rev)
    assert int(best_r[0]) == top
    assert np.allclose(probs_r[0][::-1], ref[0], rtol=1e-6, atol=0)      # (the sum runs in another order: not bit for bit)


def test_bad_arguments_are_refused_before_anything_is_launched():
    from stable_ts_amd._lib import SwxError
    model, tok, feats, _, _ = _setup("tiny", "f32")
    eng = model.engine
    lang_tokens = list(tok.all_language_tokens)
    xkv = model.cross_kv(feats[:1])
    d_lang = torch.tensor(lang_tokens, dtype=torch.int32, device="cuda")
    probs = torch.full((4, len(lang_tokens)), -7.0, dtype=torch.float32, device="cuda")
    best = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(W=1, sot=tok.sot, n_lang=len(lang_tokens), lang=d_lang):
        return eng.lib.swx_detect_language(eng.h, p(xkv), W, sot, None if lang is None else p(lang), n_lang, p(probs), p(best), eng.stream)

    assert call(n_lang=0) < 0 and call(n_lang=-3) < 0
    assert call(n_lang=eng.dims.n_vocab + 1) < 0
    assert call(sot=eng.dims.n_vocab) < 0 and call(sot=-1) < 0
    assert call(lang=None) < 0
    assert call(W=eng.max_windows + 1) < 0
    torch.cuda.synchronize()
    assert bool((probs == -7.0).all()) and bool((best == -7).all()), "a refused call must not write its outputs"
    # the ids are device memory to the library: the Python owner refuses a list with an id outside the vocabulary
    with pytest.raises(IndexError):
        eng.detect_language(xkv, tok.sot, lang_tokens + [eng.dims.n_vocab])
    with pytest.raises(IndexError):
        eng.detect_language(xkv, tok.sot, [-1] + lang_tokens)
    with pytest.raises(SwxError):
        eng.detect_language(xkv, tok.sot, [])
    assert call() == 0                                                    # and the same arguments, in range, run
    torch.cuda.synchronize()
    assert abs(float(probs[0].sum()) - 1.0) <= 1e-5 and int(best[0]) in lang_tokens
