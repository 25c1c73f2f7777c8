"""Scripted-logits cases for the on-device token selection (csrc/swx_decode.hip) and their reference.

A case is a handful of logits rows per step, chosen so that a given rule of the selection path decides the next token.  The
reference (``run_reference``) does not restate a rule: it drives the oracle's own classes -- ``SuppressBlank``, ``SuppressTokens``,
``ApplyTimestampRules`` (oracle/whisper/decoding.py), ``_MinTokens`` (oracle/stable.py), ``GreedyDecoder`` / ``BeamSearchDecoder``
-- in the order and with the two extra lines (ts mask, ``nan_to_num_``) of ``oracle.stable.DecodingTaskStable._main_loop``, one
window at a time as upstream decodes.  Two expectations have no upstream counterpart and are restated here from the host code
they check, so those two comparisons are not independent of it: the number of steps executed (the loop of ``run_reference``
follows decode_loop_stop in csrc/swx_decjob.hip on the steps at which the reference's windows ended) and ``pos0`` (the last
position a window wrote, held below n_ctx).  While it runs it MEASURES, in float64, the margin of every decision (so that the f32
arithmetic of the kernels cannot legitimately flip one) and counts which rule branches the case list reaches.

Plain helper module (no fixtures, not a conftest); tests/test_select_script_cpu.py holds the conditions on the inputs,
tests/test_gpu_select_script.py runs the kernels on the same cases.

A sampling case (temperature > 0) either supplies ``noise`` (cfg.noise, the framework's Exp(1) variates) or sets ``hashed``: the
device then draws with its built-in hashed sampler (noise = NULL, cfg.seed, cfg.window_uid) and the reference is fed the float64
statement of that sampler's Exp(1) variates (tests/sampler_ref.py).
"""
import functools
from collections import Counter
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch

import sampler_ref
from oracle import stable as ost
from oracle.whisper import decoding as od

MARGIN = 1e-3          # every measured decision margin of every case must be at least this (planted exact ties excepted)
N_TS_MASK = 1501       # width of the silence mask (decode.py:14-16)

# V -> timestamp_begin.  Three real layouts (tails 664 / 665 / 666 past the last full 1024, rotation 187 / 188 / 189 of the
# timestamp sum), rotation 0, and fewer than two elements per thread with exactly 1501 timestamps
LAYOUTS = {51864: 50363, 51865: 50364, 51866: 50365, 2600: 1024, 1601: 100}
RULE_LAYOUTS = (51865, 1601)


class Tok:
    """the token ids the filters read (a stand-in for whisper.tokenizer.Tokenizer)"""

    def __init__(self, V):
        tsb = LAYOUTS[V]
        self.n_vocab, self.timestamp_begin = V, tsb
        self.no_timestamps, self.no_speech = tsb - 1, tsb - 2
        self.eot = tsb - 107 if tsb > 200 else tsb - 10
        self.sot = self.eot + 1
        self.blank = 220 if self.eot > 220 else 5

    def encode(self, text):
        assert text == " "
        return [self.blank]


@dataclass
class Case:
    name: str
    V: int
    n_ctx: int
    W: int
    G: int
    sample_len: int
    init: List[List[int]]                 # initial tokens per window
    prefill: np.ndarray                   # f32 [W][2][V]
    script: np.ndarray                    # f32 [S][W * G][V]
    beam: int = 0
    temperature: float = 0.0
    patience: float = 0.0
    min_tokens: int = 0
    suppress_blank: int = 0
    rules: int = 0
    max_initial: int = -1
    suppress: tuple = ()
    ts_mask: Optional[np.ndarray] = None  # uint8 [W][1501]
    noise: Optional[np.ndarray] = None    # f32 [sample_len][W * G][V]
    ties: set = field(default_factory=set)   # (window, step) with a planted exact tie: no margin is asked there
    hashed: bool = False                  # temperature > 0 without noise: the built-in hashed draw, keyed on seed / window_uid
    seed: int = 0                         # cfg.seed
    window_uid: Optional[tuple] = None    # cfg.window_uid [W]
    planted: Optional[tuple] = None       # (step, row, id) a case is built around
    _q: Optional[np.ndarray] = None

    blank: int = -1                       # >= 0: the id of " " where the stand-in's is not the tokenizer's

    @property
    def tok(self):
        t = Tok(self.V)
        if self.blank >= 0:
            t.blank = self.blank
        return t

    @property
    def begins(self):
        return [len(t) for t in self.init]

    def draw_q(self, w, i):
        """the Exp(1) variates [G][V] the G rows of window w draw token i with: cfg.noise, or the hashed sampler's statement"""
        if self.noise is None:
            assert self.hashed, "a sampling case gives cfg.noise or asks for the hashed draw (hashed=True): it has neither"
            if self._q is None:
                self._q = sampler_ref.job_q(self.seed, self.sample_len, self.W, self.G, self.V, self.window_uid)
            return self._q[i, w * self.G:(w + 1) * self.G]
        assert not self.hashed, "cfg.noise replaces the hashed draw: a case has one or the other"
        return self.noise[i, w * self.G:(w + 1) * self.G]

    def draw_slack(self, w, i):
        """[G][V] or None: how far the variate of each id lies from its neighbouring buckets' (hashed draw only)"""
        if not self.hashed:
            return None
        k = sampler_ref.bucket(sampler_ref.job_words(self.seed, self.sample_len, self.W, self.G, self.V, self.window_uid)[i, w * self.G:(w + 1) * self.G])
        k = k.astype(np.int64)
        g = sampler_ref.g_of_bucket
        return np.maximum(g(np.minimum(k + 1, sampler_ref.N_BUCKETS - 1)) - g(k), g(k) - g(np.maximum(k - 1, 0)))

    def logits(self, w, i):
        """the raw logits the G rows of window w select token i from"""
        if i == 0:
            return np.repeat(self.prefill[w, 1][None], self.G, 0)
        return self.script[i - 1, w * self.G:(w + 1) * self.G]


# ------------------------------------------------------------------------------------------------------------ reference
class _Inference:
    """stands where PyTorchInference stands: returns the script, records what the beam decoder asks of the KV cache"""

    def __init__(self, case, w):
        self.case, self.w, self.sources = case, w, []

    def logits(self, i):
        return torch.from_numpy(np.ascontiguousarray(self.case.logits(self.w, i))).clone()

    def rearrange_kv_cache(self, source_indices):
        self.sources.append(list(source_indices))

    def cleanup_caching(self):
        pass


class _SpyDict(dict):
    """BeamSearchDecoder's store of finished sequences, counting how often its size is asked and how often it is written: the
    decoder asks once per arriving sequence and once more when it turns one away for want of room.  Feeds the coverage counter
    `max_cand_overflow` only, never an expectation; it leans on how oracle/whisper/decoding.py is written today, and a change
    there shows as that counter staying at zero in tests/test_select_script_cpu.py"""
    n_len = n_set = 0

    def __len__(self):
        self.n_len += 1
        return dict.__len__(self)

    def __setitem__(self, k, v):
        self.n_set += 1
        dict.__setitem__(self, k, v)


class _LogSoftmaxTap:
    """stands where decoding.py's ``F`` stands while ApplyTimestampRules runs: hands the input of its log_softmax to the recorder"""

    def __init__(self):
        self.seen = []

    def log_softmax(self, x, dim=-1):
        self.seen.append(x.detach().clone())
        return torch.nn.functional.log_softmax(x, dim=dim)

    def __getattr__(self, name):
        return getattr(torch.nn.functional, name)


class _NoiseDraw:
    """stands where decoding.py's ``Categorical`` stands: the multinomial draw the framework makes from Exp(1) variates q (cfg.noise,
    or the float64 statement of the hashed sampler's), argmax_i(logits_i / T - log q_i), in float64.  The margin it measures is
    that of the winner's key LESS its slack over every other key PLUS its slack: no slack with cfg.noise (the device reads the
    same f32 numbers); for the hashed draw, the distance to the neighbouring buckets' variates -- what the f32 variate of the
    device may be off by (one bucket: tests/test_gpu_sampler.py), next to nothing mid-range and up to 1.1 in the outermost
    buckets, so that no case leans on a draw from the far tails"""
    noise = None
    slack = None
    margins = None

    def __init__(self, logits):
        self.key = logits.double() - torch.log(torch.from_numpy(np.ascontiguousarray(_NoiseDraw.noise)).double())

    def sample(self):
        pick = self.key.argmax(dim=-1)
        slack = torch.zeros_like(self.key) if _NoiseDraw.slack is None else torch.from_numpy(np.ascontiguousarray(_NoiseDraw.slack))
        rows = torch.arange(self.key.shape[0])
        others = self.key + slack
        others[rows, pick] = -np.inf
        _NoiseDraw.margins.extend(((self.key[rows, pick] - slack[rows, pick]) - others.max(dim=-1).values).tolist())
        return pick


@dataclass
class Ref:
    tokens: np.ndarray        # int32 [W][G_out][n_ctx + 1], eot padded (unused slots: all eot)
    lens: np.ndarray          # int32 [W][G_out], -1 = unused slot
    sumlp: np.ndarray         # f64 [W][G_out] (unused slots: nan)
    nospeech: np.ndarray      # f64 [W]
    steps: int
    anc: Optional[np.ndarray]  # int32 [M][n_ctx] (G > 1)
    pos0: np.ndarray          # int32 [M]
    margins: list             # (what, window, step, value)
    counts: Counter


def g_out(case):
    if not case.beam:
        return case.G
    return max(case.G, round(case.G * (case.patience or 1.0)))


def _finite_gaps(v):
    v = np.sort(np.asarray(v, np.float64))[::-1]
    return (v[:-1] - v[1:]).tolist()


def _run_window(case, w, counts, margins):
    tok, G, V, n_ctx = case.tok, case.G, case.V, case.n_ctx
    tsb, n0 = tok.timestamp_begin, case.begins[w]
    inference = _Inference(case, w)
    filters = []
    if case.suppress_blank:
        filters.append(od.SuppressBlank(tok, n0))
    if case.suppress:
        filters.append(od.SuppressTokens(case.suppress))
    if case.min_tokens:
        filters.append(ost._MinTokens(tok.eot, n0, case.min_tokens))
    rules = od.ApplyTimestampRules(tok, n0, None if case.max_initial < 0 else case.max_initial) if case.rules else None
    if rules:
        filters.append(rules)
    if case.beam:
        decoder = od.BeamSearchDecoder(G, tok.eot, inference, case.patience or None)
        decoder.finished_sequences = [_SpyDict()]
    else:
        decoder = od.GreedyDecoder(case.temperature, tok.eot)
    mask = None if case.ts_mask is None else torch.from_numpy(case.ts_mask[w].astype(bool))
    tokens = torch.tensor([case.init[w]]).repeat(G, 1)
    sum_lp = torch.zeros(G)
    at_sot = torch.from_numpy(case.prefill[w, 0]).float().softmax(dim=-1)
    nospeech = at_sot[tok.no_speech].item()
    anc = np.repeat(np.where(np.arange(n_ctx) < n0, w * G, 0)[None], G, 0)
    for g in range(G):
        anc[g, n0:] = w * G + g
    tied = lambda i: (w, i) in case.ties
    note = lambda what, i, v: margins.append((what, w, i, float(v)))
    last = 0
    for i in range(case.sample_len):
        last = i
        logits = inference.logits(i)
        raw = logits.clone()
        seq = tokens[0, n0:].tolist()
        for f in filters:
            if f is rules:
                before = logits.clone()
                tap = _LogSoftmaxTap()
                od.F, keep = tap, od.F
                try:
                    f.apply(logits, tokens)
                finally:
                    od.F = keep
                _note_rules(case, w, i, tokens[:, n0:], before, tap.seen[0], logits, counts, note, tied(i))
            else:
                f.apply(logits, tokens)
        if mask is not None:
            pick = logits.nan_to_num(-np.inf).argmax(dim=-1)
            logits[:, tsb:][:, mask] = -np.inf
            if case.rules and (pick != logits.nan_to_num(-np.inf).argmax(dim=-1)).any():
                counts["ts_mask"] += 1                       # (with the rules on: the setting production masks in)
            if case.rules and not torch.isfinite(logits).any():
                counts["ts_mask_strikes_whole_row"] += 1
        for name, hit in (("nan", torch.isnan(logits)), ("pinf", logits == np.inf), ("ninf", raw == -np.inf)):
            if hit[:, :tsb].any():
                counts[name + "_text"] += 1
            if hit[:, tsb:].any():
                counts[name + "_ts"] += 1
        logits.nan_to_num_(-np.inf)
        if i == 0 and case.suppress_blank and raw[0].argmax().item() in (tok.blank, tok.eot):
            counts["suppress_blank"] += 1
        if i > 0 and case.suppress_blank and raw[0].argmax().item() == tok.blank == logits[0].argmax().item():
            counts["blank_allowed_later"] += 1
        if case.suppress and raw[0, list(case.suppress)].max() > raw[0, logits[0].argmax()]:
            counts["suppress_list"] += 1
        if case.min_tokens and raw[0].argmax().item() == tok.eot:
            counts["min_tokens_on" if i < case.min_tokens else "min_tokens_lifted"] += 1
        if case.beam:
            _note_beam(case, i, tokens, logits, sum_lp, note, tied(i))
            store = decoder.finished_sequences[0]
            had, store.n_len, store.n_set = dict.__len__(store), 0, 0
            tokens, completed = decoder.update(tokens, logits, sum_lp)
            if store.n_len - store.n_set - 1 > 0:          # (- 1: the completion test asks once)
                counts["max_cand_overflow"] += 1
            if dict.__len__(store) > had:
                counts["beam_finished"] += 1
            if completed and (case.patience or 1.0) > 1.0:
                counts["patience_max_cand"] += 1
            src, old, n = inference.sources[-1], anc.copy(), n0 + i
            for g in range(G):
                anc[g, :n] = old[src[g], :n]
                anc[g, n:] = w * G + g
        else:
            live = tokens[:, -1] != tok.eot
            if case.temperature == 0:
                top = logits.double().topk(2, dim=-1).values
                for g in range(G):
                    if live[g] and not tied(i):
                        note("argmax", i, top[g, 0] - top[g, 1])
            else:
                _NoiseDraw.noise, _NoiseDraw.slack, _NoiseDraw.margins = case.draw_q(w, i), case.draw_slack(w, i), []
            if (~live).any() and live.any():
                counts["row_past_eot"] += 1
            od.Categorical, keep = _NoiseDraw, od.Categorical
            try:
                tokens, completed = decoder.update(tokens, logits, sum_lp)
            finally:
                od.Categorical = keep
            if case.temperature != 0:
                for g in range(G):
                    if live[g] and not tied(i):
                        note("draw", i, _NoiseDraw.margins[g])
        if completed or tokens.shape[-1] > n_ctx:
            done = "completed" if completed else "ctx_full"
            break
    else:
        done = "budget"
    inference.cleanup_caching()
    live_lp = sum_lp.clone()
    n_finished = dict.__len__(decoder.finished_sequences[0]) if case.beam else 0
    out_tok, out_lp = decoder.finalize(tokens.reshape(1, G, -1), sum_lp.reshape(1, G))
    if case.beam:
        seqs, lps = [t.tolist() for t in out_tok[0]], list(out_lp[0])
    else:
        seqs, lps = out_tok[0].tolist(), list(out_lp[0])
    return dict(seqs=seqs, lps=lps, nospeech=nospeech, anc=anc, last=last, done=done, live_lp=live_lp,
                n_finished=n_finished)


def _note_rules(case, w, i, sampled, before, compared, after, counts, note, tied):
    """what ApplyTimestampRules did to the rows of one step: counted from the token history and from the rows before / after, and
    the margin of its comparison measured on the very tensor it took the log-softmax of"""
    tok = case.tok
    tsb = tok.timestamp_begin
    for g in range(sampled.shape[0]):
        seq = sampled[g].tolist()
        if seq and seq[-1] == tok.eot:
            continue
        ts = [t for t in seq if t >= tsb]
        last_ts = bool(seq) and seq[-1] >= tsb
        pen_ts = len(seq) < 2 or seq[-2] >= tsb
        if not ts:
            counts["no_timestamp_yet"] += 1
        if last_ts and pen_ts:
            counts["pair_ts_ts"] += 1
        elif last_ts:
            counts["pair_text_ts"] += 1
        elif len(seq) >= 2 and seq[-2] >= tsb:
            counts["hist_ts_text"] += 1
        if ts:
            open_pair = last_ts and not pen_ts
            counts["mono_tl" if open_pair else "mono_tl_plus_1"] += 1
            if open_pair and after[g].nan_to_num(-np.inf).argmax().item() == ts[-1]:
                counts["repeat_allowed"] += 1
            if before[g].nan_to_num(-np.inf).argmax().item() == ts[-1] and not torch.isfinite(compared[g, ts[-1]]):
                counts["repeat_forbidden"] += 1
        if not seq and case.max_initial >= 0:
            cut = torch.isfinite(before[g, tsb + case.max_initial + 1:]) & ~torch.isfinite(compared[g, tsb + case.max_initial + 1:])
            if cut.any() and before[g, tsb:].argmax().item() > case.max_initial:
                counts["max_initial_cut"] += 1
        x = compared[g].double()
        if seq and torch.isfinite(x[:tsb]).any():      # (step 0 has no text left to suppress)
            if torch.isnan(x).any() or (x == np.inf).any():
                counts["compare_nonfinite"] += 1
                assert torch.isfinite(after[g, :tsb]).any() or not torch.isfinite(compared[g, :tsb]).any()
            else:
                gap = x[tsb:].logsumexp(dim=-1) - x[:tsb].max()
                suppressed = not torch.isfinite(after[g, :tsb]).any()
                counts["text_suppressed" if suppressed else "text_kept"] += 1
                if torch.isfinite(x[tsb:]).any() and not tied:
                    note("ts_vs_text", i, abs(gap.item()))
                    if torch.isfinite(x[:tsb]).sum() > 0 and torch.isfinite(x[tsb:]).sum() > 1 and x[tsb:].max() < x[:tsb].max():
                        counts["ts_mass_beats_single_text" if suppressed else "ts_mass_loses"] += 1


def _note_beam(case, i, tokens, logits, sum_lp, note, tied):
    """margins of one beam step: the top-(G + 1) of every row (order and membership) and the ranking of all candidates"""
    if tied:
        return
    G = case.G
    lp = torch.log_softmax(logits.double(), dim=-1)
    rows = range(1) if i == 0 else range(G)            # all rows hold the same sequence and logits at the first step
    scores = []
    for j in rows:
        top = lp[j].topk(G + 2)
        assert (logits[j] > -1e30).sum() >= G + 2, "a beam row needs G + 2 unmasked tokens"
        for gap in (top.values[:-1] - top.values[1:]).tolist():
            note("topk", i, gap)
        scores += (sum_lp[j].double() + top.values[:G + 1]).tolist()
    for gap in _finite_gaps(scores):
        note("beam_rank", i, gap)


def run_reference(case) -> Ref:
    tok, W, G, n_ctx = case.tok, case.W, case.G, case.n_ctx
    TS, Go = n_ctx + 1, g_out(case)
    counts, margins = Counter(), []
    tokens = np.full((W, Go, TS), tok.eot, np.int32)
    lens = np.full((W, Go), -1, np.int32)
    sumlp = np.full((W, Go), np.nan)
    nospeech = np.zeros(W)
    anc = np.zeros((W * G, n_ctx), np.int32)
    pos0 = np.zeros(W * G, np.int32)
    wins = [_run_window(case, w, counts, margins) for w in range(W)]
    begins = case.begins
    ragged = min(begins) != max(begins)
    for w, r in enumerate(wins):
        for k, (s, p) in enumerate(zip(r["seqs"], r["lps"])):
            tokens[w, k, :len(s)] = s[:TS]
            row = list(tokens[w, k, begins[w]:]) + [tok.eot]
            lens[w, k] = row.index(tok.eot)
            sumlp[w, k] = p
        nospeech[w] = r["nospeech"]
        anc[w * G:(w + 1) * G] = r["anc"]
        pos0[w * G:(w + 1) * G] = min(begins[w] + r["last"], n_ctx - 1)
        if case.beam and r["n_finished"] < G:
            counts["finalize_top_up"] += 1
            for gap in _finite_gaps(r["live_lp"].tolist()):
                margins.append(("top_up", w, r["last"], gap))
        if case.beam and len(r["seqs"]) < Go:
            counts["unused_slot"] += 1
        if r["done"] == "ctx_full":
            counts["ctx_full_ragged" if ragged else "ctx_full_uniform"] += 1
    # the host loop's exits (swx_decjob.hip: decode_loop_stop) on the steps at which the windows ended
    end = [r["last"] if r["done"] != "budget" else None for r in wins]
    steps = 0
    for i in range(case.sample_len):
        steps = i + 1
        if min(begins) + i + 1 > n_ctx:
            break
        if (steps % 8 == 0 and steps >= case.min_tokens) or steps == case.sample_len:
            if all(e is not None and e <= i for e in end):
                break
        if steps >= case.sample_len:
            break
    if steps < case.sample_len and min(begins) + steps <= n_ctx:
        counts["poll_exit"] += 1
    assert all(r["last"] <= steps - 1 for r in wins)
    if any(e is not None and e < steps - 1 for e in end) and any(r["last"] > min(e for e in end if e is not None) for r in wins):
        counts["early_window_freeze"] += 1
    if any(e is not None and e < steps - 1 for e in end):
        counts["steps_past_completion"] += 1
    return Ref(tokens, lens, sumlp, nospeech, steps, anc if G > 1 else None, pos0, margins, counts)


# ---------------------------------------------------------------------------------------------------------------- cases
HI, OK = 15.0, 12.0        # a tempting logit that a rule must strike out / the best logit that stays allowed


def _base(V, W, G, n_script, seed):
    """distinct-looking background in [-4, 0): a single one never decides anything, the 1501 timestamps together weigh
    logsumexp ~ 5.9"""
    rng = np.random.default_rng(seed)
    prefill = rng.uniform(-4, 0, (W, 2, V)).astype(np.float32)
    script = rng.uniform(-4, 0, (n_script, W * G, V)).astype(np.float32)
    return rng, prefill, script


def _init(tok, n):
    return [tok.sot] + [tok.sot + 2 + k for k in range(n - 1)]


def _row(case_arrays, w, G, i, g=None):
    """the logits row(s) token i of window w is selected from (a view to plant into)"""
    prefill, script = case_arrays
    if i == 0:
        return prefill[w, 1]
    return script[i - 1, w * G:(w + 1) * G] if g is None else script[i - 1, w * G + g]


def case_rules(V, max_initial, seed=1):
    """one greedy row through every timestamp rule: each step tempts with a logit the rule must strike out (HI) next to the best
    allowed one (OK)"""
    tok = Tok(V)
    tsb, A, B, D, E = tok.timestamp_begin, 300 % tok.eot, 1100 % tok.eot, 17, 41
    rng, prefill, script = _base(V, 1, 1, 9, seed)
    R = lambda i: _row((prefill, script), 0, 1, i, 0)
    c = tsb + 70
    R(0)[A] = HI; R(0)[tsb + 60] = 14.0; R(0)[tsb + 10] = OK; R(0)[tsb] = 5.0        # first token: a timestamp, <= max_initial
    R(1)[tsb + 200] = HI; R(1)[tok.no_timestamps] = 14.0; R(1)[A] = OK                 # ts, (ts): text next
    R(2)[tsb + 60 if max_initial < 0 else tsb] = HI; R(2)[B] = OK                      # ts, text: the last timestamp not again
    R(3)[tsb + 5 if max_initial != 0 else tsb] = HI; R(3)[c] = OK                      # text, text: a later timestamp
    R(4)[A] = HI; R(4)[c] = OK; R(4)[c + 1] = 9.0                                      # text, ts: no text; the same timestamp may repeat
    R(5)[c] = HI; R(5)[c + 9] = 14.0; R(5)[D] = OK                                     # ts, ts (identical): no timestamp at all
    R(6)[c] = HI; R(6)[E] = 8.0; R(6)[c + 30] = 1.0                                    # now c is forbidden; text 8.0 beats the timestamp mass
    R(7)[E] = 5.0; R(7)[c + 40] = 1.0                                                  # the mass of ~1400 timestamps beats a single text 5.0
    R(8)[A] = HI; R(8)[tok.eot] = OK                                                   # text, ts: EOT closes
    return Case(f"rules_mi{max_initial}_V{V}", V, 16, 1, 1, 10, [_init(tok, 3)], prefill, script, rules=1,
                max_initial=max_initial, suppress_blank=1)


def case_filters(V, seed=2):
    """rules off: blank and EOT struck at step 0 only, a suppress list, min_tokens on and at the step it lifts"""
    tok = Tok(V)
    sup = (7, 23, tok.sot, tok.no_speech)
    rng, prefill, script = _base(V, 1, 1, 7, seed)
    R = lambda i: _row((prefill, script), 0, 1, i, 0)
    R(0)[tok.blank] = HI; R(0)[tok.eot] = 14.5; R(0)[23] = 14.0; R(0)[60] = OK
    R(1)[tok.blank] = HI; R(1)[61] = OK                       # the blank is allowed again
    R(2)[tok.eot] = HI; R(2)[7] = 14.0; R(2)[62] = OK
    R(3)[tok.eot] = HI; R(3)[63] = OK                         # 3 < min_tokens
    R(4)[tok.eot] = HI; R(4)[64] = OK                         # lifted
    return Case(f"filters_V{V}", V, 12, 1, 1, 8, [_init(tok, 4) + [tok.no_timestamps]], prefill, script, suppress_blank=1,
                suppress=sup, min_tokens=4)


def case_ties(V, seed=3):
    """exact equal maxima: same thread (i, i + 1024), neighbours, the wave edge, both ends of the row, the stride edge"""
    tok = Tok(V)
    pairs = [(37, 37 + 1024), (70, 71), (63, 64), (0, V - 1), (1023, 1024)]
    rng, prefill, script = _base(V, 1, 1, len(pairs) - 1, seed)
    for i, (a, b) in enumerate(pairs):
        row = _row((prefill, script), 0, 1, i, 0)
        row[a] = row[b] = OK
    return Case(f"ties_V{V}", V, 12, 1, 1, len(pairs), [_init(tok, 2)], prefill, script,
                ties={(0, i) for i in range(len(pairs))})


def case_ts_mask(V, everything, seed=4):
    """the silence mask together with the timestamp rules, as production sets it.  History (ts, text, text), then a row whose
    timestamp mass (~5.9) beats the best text (5.0): the rules strike the text on the UNMASKED timestamps' mass, and only then the
    mask strikes the timestamp they would pick (tsb + 400) and the next best, the mask's last entry (tsb + 1500): tsb + 410 is
    left.  Window 1 masks its own pattern and ends on the last timestamp.  `everything`: window 0 masks all 1501 -- the text goes
    (the mass is still counted), then every timestamp: the row is one value throughout and index 0 wins (steps 0 and 3, planted
    ties).  A kernel that applied the mask before the comparison would keep the text there"""
    tok = Tok(V)
    tsb = tok.timestamp_begin
    assert V - tsb == N_TS_MASK
    rng, prefill, script = _base(V, 2, 1, 4, seed)
    mask = np.zeros((2, N_TS_MASK), np.uint8)
    for w in range(2):
        R = lambda i: _row((prefill, script), w, 1, i, 0)
        R(0)[tsb + 10] = OK
        R(1)[30] = OK
        R(2)[31] = OK
        R(3)[32] = 5.0; R(3)[tsb + 400] = 1.0; R(3)[tsb + 410] = 0.5; R(3)[tsb + 1500] = 0.7 if w == 0 else 0.3
        R(4)[33] = OK; R(4)[tsb + 500] = 11.0; R(4)[tok.eot] = 10.0
    mask[0, 400] = mask[0, 1500] = 1
    mask[1, 400] = mask[1, 410] = 1
    ties = set()
    if everything:
        mask[0, :] = 1
        ties = {(0, 0), (0, 3)}
    return Case(f"ts_mask_{'all' if everything else 'pick'}_V{V}", V, 12, 2, 1, 5, [_init(tok, 3)] * 2, prefill, script,
                rules=1, ts_mask=mask, ties=ties)


def case_nonfinite(V, kind, seed=5):
    """NaN / +inf / -inf planted in the text and in the timestamp range of a row whose text-vs-timestamp comparison matters:
    history (ts, text, text), best text 5.0 below the timestamp mass.  Window 0: the text range, window 1: the timestamp range,
    window 2: both.  kind 'all': the three classes together"""
    tok = Tok(V)
    tsb = tok.timestamp_begin
    vals = {"nan": [np.nan], "pinf": [np.inf], "ninf": [-np.inf], "all": [np.nan, np.inf, -np.inf]}[kind]
    rng, prefill, script = _base(V, 3, 1, 4, seed)
    ties = set()
    for w in range(3):
        R = lambda i: _row((prefill, script), w, 1, i, 0)
        R(0)[tsb + 10] = OK
        R(1)[30] = OK
        R(2)[31] = OK
        R(3)[32] = 5.0; R(3)[tsb + 400] = 1.0
        R(4)[33] = OK; R(4)[tsb + 500] = 11.0          # (after a timestamp at step 3 the text is struck: the timestamp then)
        for k, v in enumerate(vals):
            if w in (0, 2):
                R(3)[50 + k] = v
            if w in (1, 2):
                R(3)[tsb + 300 + k] = v
        if np.inf in vals and w == 2:
            ties.add((2, 3))             # two +inf become the same largest finite value: the smaller index wins
    return Case(f"nonfinite_{kind}_V{V}", V, 12, 3, 1, 5, [_init(tok, 3)] * 3, prefill, script, rules=1, ties=ties)


def case_greedy_completion(V, seed=6):
    """window 0 picks EOT at step 2 of 11 and is frozen; window 1 runs the whole budget; the job is polled at step 8"""
    tok = Tok(V)
    rng, prefill, script = _base(V, 2, 1, 10, seed)
    for w in range(2):
        for i in range(11):
            row = _row((prefill, script), w, 1, i, 0)
            row[100 + i] = OK
            if w == 0 and i == 2:
                row[tok.eot] = HI
            if w == 0 and i > 2:
                row[100 + i] = 6.0       # log-probability about -3.5 (-0.7 at V = 1601): what a frozen window that still
                                         # accumulated would add per step
    return Case(f"greedy_eot_V{V}", V, 16, 2, 1, 11, [_init(tok, 3) + [tok.no_timestamps]] * 2, prefill, script)


def case_sampling(V, seed=7):
    """best-of 3 with cfg.noise at T = 0.5: rows end at steps 1, 3 and never-before-5; a finished row stops accumulating (its
    later rows offer a 6.0 of log-probability about -3.5, -0.7 at V = 1601, which would show in the sum); the noise overturns the
    arg-max of the logits once"""
    tok = Tok(V)
    G, S = 3, 6
    rng, prefill, script = _base(V, 1, G, S - 1, seed)
    noise = rng.uniform(0.6, 1.6, (S, G, V)).astype(np.float32)
    prefill[0, 1, 80] = 6.0; prefill[0, 1, 81] = 5.8
    noise[0, :, 80] = 1.5; noise[0, 1, 81] = 0.3          # row 1: 2 * 5.8 - log 0.3 beats 2 * 6.0 - log 1.5
    noise[0, 0, 81] = noise[0, 2, 81] = 1.5
    for i in range(1, S):
        for g in range(G):
            row = script[i - 1, g]
            row[90 + i] = 6.0
            if (g, i) in ((0, 1), (2, 3)):
                row[tok.eot] = 8.0
    return Case(f"sampling_V{V}", V, 12, 1, G, S, [_init(tok, 3) + [tok.no_timestamps]], prefill, script, temperature=0.5,
                noise=noise)


HASH_HI = 0x5BD1E995       # high half of the hashed cases' cfg.seed: both halves are non-zero
UIDS = (7, 3_000_000)      # window uids of the uid-keyed variants
# low half of cfg.seed per (V, T, keyed): counted up from 1 on the CPU until the reference alone meets the margin condition
# (tests/test_select_script_cpu.py); default 1
_HASH_LO = {}


def case_hashed_sampling(V, T, window_uid=None, seed=12):
    """best-of 3 in two windows drawn by the BUILT-IN hashed sampler (noise = NULL on the device): every row offers eight tokens
    within 1.0 of one another above the background, so that at T = 1 the draw spreads over all eight (and now and then over the
    background), at T = 0.2 over the best few; two rows are offered EOT on the way and stop accumulating where they take it"""
    tok = Tok(V)
    W, G, S = 2, 3, 6
    rng, prefill, script = _base(V, W, G, S - 1, seed)
    pool = np.arange(260, tok.eot - 1) if tok.eot > 400 else np.arange(tok.timestamp_begin + 10, V - 10)
    for w in range(W):
        for i in range(S):
            for g in range(1 if i == 0 else G):
                row = _row((prefill, script), w, G, i, None if i == 0 else g)
                row[rng.choice(pool, 8, replace=False)] = rng.uniform(11.0, 12.0, 8).astype(np.float32)
                if (w, g, i) in ((0, 0, 1), (1, 2, 3)):
                    row[tok.eot] = 14.0
    keyed = window_uid is not None
    lo = _HASH_LO.get((V, T, keyed), 1)
    return Case(f"hashed_T{T}{'_uid' if keyed else ''}_V{V}", V, 12, W, G, S, [_init(tok, 3) + [tok.no_timestamps]] * W, prefill,
                script, temperature=T, hashed=True, seed=(HASH_HI << 32) | lo, window_uid=window_uid)


LEAD = 18.0                # the clear lead of the top-bucket cases: a background token (< 0) would need a variate 18 above the lead's


@functools.lru_cache(maxsize=None)
def _top_bucket_tuple(V):
    """(seed, step, row, id): the first seed HASH_HI << 32 | 1, 2, ... under which a (step <= 4, row < 6, id < V) of a 2 x 3 job
    draws the TOP bucket of the hashed sampler -- and the id is no token the case needs for itself"""
    tok = Tok(V)
    lo = 1
    while True:
        hit = sampler_ref.find_top_bucket(5, 2, 3, V, 4, range(lo, 1 << 20), hi=HASH_HI)
        assert hit is not None
        if hit[3] not in (tok.eot, 7, 300, 301):
            return hit
        lo = (hit[0] & 0xFFFFFFFF) + 1


def case_top_bucket(V, suppressed, seed=13):
    """the hashed draw's top bucket (u nearest 1, the largest variate: 17.33 by the contract) falls on a token that must not win:
    id X of one row at one step, at T = 1, while token 300 leads that row by far.  `suppressed`: X is on the suppress list (masked,
    no variate may lift it); otherwise X is allowed but 30 below the lead, more than any finite variate spans (-2.86 .. 17.33).
    A sampler whose top bucket is not finite selects X"""
    tok = Tok(V)
    W, G, S = 2, 3, 5
    hseed, step, row, x = _top_bucket_tuple(V)
    rng, prefill, script = _base(V, W, G, S - 1, seed)
    for w in range(W):
        for i in range(S):
            r = _row((prefill, script), w, G, i)
            r[..., 300 + (i & 1)] = LEAD
            if not suppressed and w == row // G:
                if i == 0 and step == 0:
                    r[x] = LEAD - 30.0            # (step 0: the window's rows share the prefill row)
                elif i == step and i > 0:
                    r[row % G, x] = LEAD - 30.0
    return Case(f"top_bucket_{'suppressed' if suppressed else 'far_below'}_V{V}", V, 12, W, G, S,
                [_init(tok, 3) + [tok.no_timestamps]] * W, prefill, script, temperature=1.0, hashed=True, seed=hseed,
                suppress=(7, x) if suppressed else (), planted=(step, row, x))


# seeds chosen on the CPU until the reference alone meets the margin condition (tests/test_select_script_cpu.py); default 8
_BEAM_SEED = {("_b", 5, 1.0, 51865): 9, ("_c", 5, 1.0, 51865): 10, ("_c", 5, 1.0, 1601): 17, ("_b", 5, 2.0, 1601): 55}


def case_beam(V, G, patience, eot_plan, W=1, sample_len=5, seed=8, n_ctx=14, tag=""):
    """beam search on rows that each offer G + 2 comparable tokens; eot_plan {(window, step): rows} puts EOT on top of those rows"""
    tok = Tok(V)
    seed = _BEAM_SEED.get((tag, G, patience, V), seed)
    rng, prefill, script = _base(V, W, G, sample_len - 1, seed)
    pool = np.arange(260, tok.eot - 1) if tok.eot > 400 else np.arange(tok.timestamp_begin + 10, V - 10)
    for w in range(W):
        for i in range(sample_len):
            for g in range(1 if i == 0 else G):
                row = _row((prefill, script), w, G, i, None if i == 0 else g)
                ids = rng.choice(pool, G + 2, replace=False)
                row[ids] = (OK + np.sort(rng.uniform(0, 3.0, G + 2))[::-1] + 0.05 * np.arange(G + 2)[::-1]).astype(np.float32)
                if g in eot_plan.get((w, i), ()):
                    row[tok.eot] = OK + 6.0
    return Case(f"beam{tag}_G{G}_p{patience}_V{V}", V, n_ctx, W, G, sample_len, [_init(tok, 3) + [tok.no_timestamps]] * W,
                prefill, script, beam=1, patience=patience)


def case_ragged(V, seed=9):
    """sample_begins [3, 9] in a 12-token context: window 1 is full after 4 tokens and frozen, window 0 ends the job after 10"""
    tok = Tok(V)
    rng, prefill, script = _base(V, 2, 1, 9, seed)
    for w in range(2):
        for i in range(10):
            _row((prefill, script), w, 1, i, 0)[400 + 3 * i + w] = OK if w == 0 or i < 4 else 6.0
    return Case(f"ragged_V{V}", V, 12, 2, 1, 12, [_init(tok, 2) + [tok.no_timestamps], _init(tok, 8) + [tok.no_timestamps]],
                prefill, script)


def case_poll_exit(V, seed=11):
    """both windows pick EOT early (steps 1 and 3) with a budget of 12: the loop leaves at the poll after step 8"""
    tok = Tok(V)
    rng, prefill, script = _base(V, 2, 1, 11, seed)
    for w in range(2):
        for i in range(12):
            row = _row((prefill, script), w, 1, i, 0)
            row[100 + i] = OK if i <= (1, 3)[w] else 6.0
            if i == (1, 3)[w]:
                row[tok.eot] = HI
    return Case(f"poll_exit_V{V}", V, 16, 2, 1, 12, [_init(tok, 3) + [tok.no_timestamps]] * 2, prefill, script)


def case_ctx_exact(V, G, beam, seed=10):
    """a uniform job whose last token lands on position n_ctx: begin 4, context 12, token 8 is the ninth"""
    tok = Tok(V)
    if beam:
        c = case_beam(V, G, 1.0, {}, W=1, sample_len=10, n_ctx=12, tag="_ctx")
        c.init = [_init(tok, 3) + [tok.no_timestamps]]
        return c
    rng, prefill, script = _base(V, 1, G, 9, seed)
    for i in range(10):
        row = _row((prefill, script), 0, G, i)
        row[..., 500 + i] = OK
    return Case(f"ctx_exact_V{V}", V, 12, 1, G, 10, [_init(tok, 3) + [tok.no_timestamps]], prefill, script)


def all_cases():
    """every case, built afresh (tens of MB at the real vocabulary sizes: iterate, do not keep)"""
    for V in RULE_LAYOUTS:
        for mi in (-1, 0, 50):
            yield lambda V=V, mi=mi: case_rules(V, mi)
        yield lambda V=V: case_filters(V)
        yield lambda V=V: case_ties(V)
        yield lambda V=V: case_ts_mask(V, False)
        yield lambda V=V: case_ts_mask(V, True)
        for kind in ("nan", "pinf", "ninf", "all"):
            yield lambda V=V, kind=kind: case_nonfinite(V, kind)
        yield lambda V=V: case_greedy_completion(V)
        yield lambda V=V: case_sampling(V)
        for T in (0.2, 1.0):
            yield lambda V=V, T=T: case_hashed_sampling(V, T)
        yield lambda V=V: case_hashed_sampling(V, 1.0, UIDS)
        yield lambda V=V: case_top_bucket(V, True)
        yield lambda V=V: case_top_bucket(V, False)
        # (a) a window completes early and is frozen, (b) fewer than G finish, (c) more EOT arrive than there is room for
        yield lambda V=V: case_beam(V, 2, 1.0, {(0, 2): (0, 1)}, W=2, sample_len=6, tag="_a")
        yield lambda V=V: case_beam(V, 5, 1.0, {(0, 1): (0,)}, tag="_b")
        yield lambda V=V: case_beam(V, 5, 1.0, {(0, 1): (0, 1, 2), (0, 2): (0, 1, 2)}, W=2, sample_len=6, tag="_c")
        yield lambda V=V: case_beam(V, 2, 2.0, {(0, 1): (0, 1), (0, 2): (0,), (0, 3): (0, 1)}, W=2, sample_len=6, tag="_c")
        yield lambda V=V: case_beam(V, 2, 2.0, {(0, 2): (1,)}, tag="_b")
        yield lambda V=V: case_beam(V, 5, 2.0, {(0, 1): (0, 1), (0, 3): (2,)}, W=2, tag="_b")
        yield lambda V=V: case_ragged(V)
        yield lambda V=V: case_poll_exit(V)
        yield lambda V=V: case_ctx_exact(V, 1, 0)
        yield lambda V=V: case_ctx_exact(V, 2, 1)
    for V in (51864, 51866, 2600):
        yield lambda V=V: case_ties(V)
        yield lambda V=V: case_rules(V, -1)                   # holds the text-vs-timestamp comparison, won and lost
        yield lambda V=V: case_beam(V, 2, 1.0, {(0, 2): (0, 1)}, W=2, sample_len=6, tag="_a")


