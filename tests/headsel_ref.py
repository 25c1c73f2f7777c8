"""Float64 statement of the head-selection word stage (csrc/swx_headsel.hip: headsel_score / headsel_pick / headsel_gather,
newal_head / newal_pick / newal_mean, weighted_sum; csrc/swx_align.hip for the z-normalisation that follows the gather) and the
inputs its tests run on.  numpy only: no GPU, no library.

Contract (stable_whisper/timing.py:87-110 for ``dynamic``, :136-161 for ``new``, :177-189 for ``pool``).  A case holds the captured
queries q [L][W][max_n][d] and the cross-K k [L][W][1500][d] as values already rounded to its dtype; head ``l * H + h`` of window
``w`` scores row ``i`` against frame ``f`` with ``s = 0.125 * q[l, w, i, h*64:(h+1)*64] . k[l, w, f, h*64:(h+1)*64]``.

``dynamic``: text rows ``n_sot .. n_tok - 2``; ``p = softmax_f(s * qk_scale)`` over ``[0, F)``; peak = the lowest-index argmax of the
row, or ``j[i] + (j[i+1] - j[i]) / 2`` with the previous jumps ``j`` padded by ``F``; head score = ``sum_f |peak - f| / 1500 * p``; per
row the ``count`` smallest scores ascending, the lowest head first on a tie; the raw rows of the picks (slot k of every row) are
softmaxed again, z-normalised over the token axis with the population std per slot, median-filtered along the frames (reflect
padding, unchanged when ``F <= width / 2``) and averaged over the slots; the result is negated.

``new``: all ``n_tok`` rows; crop to ``F``, median along the frames, ``* qk_scale``, softmax; column norms over all rows, row norms,
coverage penalty ``sum_f max(sum_i p, 0.5) - 0.5 F``, each weighted only when its weight is ``> 0``; the ``topk`` largest scores,
the lowest head first on a tie; mean over the picks of ``p / column norm`` on rows ``n_sot .. n_tok - 2``, negated.

Inputs.  q rows ``>= n_tok[w]`` and K rows ``>= n_frames[w]`` are NaN (the GPU test also poisons the V^T / packed part of every
K chunk and the chunks outside a sub-batch): the reference is finite on them, a kernel that reads one row too far is not.  Random
q (one gain per (window, head, row), so head scores spread) against random K; a few heads per window are PLANTED: their q of
text row i is aligned with the key of the row's expected frame, with a peak logit of 7 .. 11 -- their scores span an order of
magnitude, as a trained model's alignment heads do.  The builder redraws single q vectors until the conditions below hold
(``violations``), then asserts them: where the peak is the row's own argmax, the two largest scaled logits of every (window, head,
text row) differ by >= 100 raw-score tolerances; consecutive head scores of the first ``count + 1`` / ``topk + 1`` ranks differ by
>= 100 score tolerances; every token-axis std is >= 1e-12 (and >= 8 u times the column's largest probability: the rows of no
column are equal in f32, where the z-score is 0 / 0) and every probability a normal f32 number.  The only exceptions are the
planted exact ties, listed in ``Case.ties``: a frame pair with identical K rows, a head made the copy of another, and the
one-frame windows of ``new`` (every head has p = 1 there: all scores are equal).

Tolerances: ``u = 2^-24`` times a condition magnitude the reference computes alongside.
  raw score        32 u A,  A = 0.125 sum_e |q_e| |k_e|
  probability      eps = (64 max_f A * qk_scale + 24) u relative (softmax of logits that are off by the raw tolerance, expf, the sum)
  dynamic score    eps * score
  z-score          (eps' p + dmu + |z| dsd) / std + 4 u |z|, eps' = eps + 4 u, dmu = mean_i eps' p, dsd = max_i eps' p + dmu
  dynamic matrix   mean over the slots of the running maximum of the z tolerance over the median's window + (count + 2) u |ref|
  column norm      (max_i eps + (n + 4) u) * norm
  'new' score      (max_i eps + (n + 24) u) * (w_col sum norm + w_row sum rownorm + w_cov sum_{cov > 0.5} cov)
                   + 16 u w_cov (sum max(cov, 0.5) + 0.5 F)
  'new' matrix     mean_k (p_k / norm_k) (eps_k,i + column-norm tolerance_k + (topk + 4) u)
  pool             4 n_in u sum_j |c_j x_j|  (n_in roundings of at most u each is the a-priori bound of the product sum)
The constants come from the formulas (64 fused multiply-adds, a 256-thread tree over <= 6 strided terms, expf and a division);
an f32 restatement of the same formulas in numpy stays below a quarter of every one of them (tests/test_headsel_ref_cpu.py), and
every mutation in MUTATIONS lands above.  Worst ratio |f32 restatement - f64| / tolerance over all cases:

  quantity   gathered  dscore  matrix(dynamic)  colnorm  nscore  matrix(new)  pool
  worst      0.211     0.104   0.021            0.092    0.013   0.029        0.249
(the pool's 0.249 is the bound itself: one f32 rounding of a single product is at most u, a quarter of 4 u).  The kernels'
ratios on an MI355X are recorded in profiles/headsel_ref_ratios.json.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

N_AUDIO_CTX = 1500
HS_MAXF = 1536
U32 = 2.0 ** -24
C_RAW = 32.0
GAP = 100.0
TINY = 1e-30
WIDE_HIGH = (256, 257, 258, 260, 261, 263)      # wide configuration (264 heads): where heads past the first 256 are planted ...
WIDE_TWINS = (259, 262)                         # ... and the two that are made copies of planted heads below 256

MUTATIONS = {
    "dynamic": ("peak_highest_on_tie", "dist_from_peak_plus_1", "softmax_all_frames", "rows_plus_1", "rows_minus_1", "head_h_L_plus_l",
                "largest_picks", "k_of_previous_window", "peaks_without_midpoint", "sample_std", "score_without_qk_scale"),
    "new": ("median_after_softmax", "crop_after_median", "symmetric_padding", "colnorm_text_rows", "rownorm_without_sqrt",
            "coverage_without_clamp", "coverage_without_half_F", "smallest_picks", "mean_over_LH", "out_rows_plus_1"),
}
QUANTITIES = {"dynamic": ("gathered", "dscore", "sel", "matrix"), "new": ("colnorm", "nscore", "top", "matrix")}


@dataclass
class Case:
    name: str
    kind: str                   # 'dynamic' | 'new'
    f16: bool
    L: int
    H: int
    n_sot: int
    n_tok: tuple                # per window
    n_frames: tuple
    max_n: int
    q: np.ndarray               # [L][W][max_n][d] storage precision, every entry finite (the mutation checks read these)
    k: np.ndarray               # [L][W][1500][d]
    opts: dict                  # dynamic: count, width, qk_scale, peaks ('own' | 'mid'); new: topk, width, qk_scale, w_col, w_row, w_cov
    jumps: Optional[list] = None            # 'mid': per window the previous pass's jump frames (ascending ints)
    planted: list = field(default_factory=list)   # per window: {head: peak logit}
    ties: dict = field(default_factory=dict)      # 'frames': (w, f1, f2) | 'heads': [(a, b)] b a copy of a | 'one_frame': [w]
    xkv_W: int = 0              # windows of the K buffer the GPU test cuts the case's windows from (0 = W) ...
    window0: int = 0            # ... starting at this one
    redrawn: int = 0

    @property
    def W(self):
        return len(self.n_tok)

    @property
    def LH(self):
        return self.L * self.H

    @property
    def d(self):
        return 64 * self.H

    @property
    def dtype(self):
        return np.float16 if self.f16 else np.float32

    def rows(self, w):
        return self.n_tok[w] - self.n_sot - 1

    @property
    def max_rows(self):
        return self.max_n - self.n_sot - 1

    def peaks(self, w, midpoint=True):
        j = np.pad(np.asarray(self.jumps[w]), (0, 1), constant_values=self.n_frames[w])
        return j[:-1] + ((j[1:] - j[:-1]) * 0.5) if midpoint else j[:-1].astype(np.float64)

    def poisoned(self):
        """(q, k) as the launch gets them: everything the contract does not read is NaN"""
        q, k = self.q.copy(), self.k.copy()
        for w in range(self.W):
            q[:, w, self.n_tok[w]:] = np.nan
            k[:, w, self.n_frames[w]:] = np.nan
        return q, k

    def matrix_compared(self, w):
        """a population std over one row is 0 and over one frame every p is 1: the reference's own z-score is 0 / 0 there"""
        return self.kind == "new" or (self.rows(w) > 1 and self.n_frames[w] > 1)


# ---------------------------------------------------------------------------------------------------------------- pieces
class _OneHead:
    L = H = 1


def raw_scores(case, q, k, w, rows, nF, dtype=np.float64, kw=None, absolute=False, heads=None):
    """[LH][len(rows)][nF]: 0.125 q . k of every head (absolute: A = 0.125 sum |q| |k|; heads: only these)"""
    L, H = case.L, case.H
    if heads is not None:
        kw = w if kw is None else kw
        out = [raw_scores(_OneHead, q[h // H:h // H + 1, :, :, h % H * 64:(h % H + 1) * 64], k[h // H:h // H + 1, :, :, h % H * 64:(h % H + 1) * 64],
                          w, rows, nF, dtype, kw, absolute) for h in heads]
        return np.concatenate(out) if out else np.zeros((0, len(rows), nF), dtype)
    qw = q[:, w][:, rows].astype(dtype).reshape(L, len(rows), H, 64).transpose(0, 2, 1, 3)
    kw = w if kw is None else kw
    if k is getattr(case, "k", None):            # the case's own K: converted once per window (the mutation checks come back for it)
        memo = case.__dict__.setdefault("_kt", {})
        if (kw, dtype) not in memo:
            memo[kw, dtype] = np.ascontiguousarray(k[:, kw].astype(dtype).reshape(L, N_AUDIO_CTX, H, 64).transpose(0, 2, 3, 1))
        kk = memo[kw, dtype][..., :nF]
    else:
        kk = k[:, kw, :nF].astype(dtype).reshape(L, nF, H, 64).transpose(0, 2, 3, 1)
    if absolute:
        qw, kk = np.abs(qw), np.abs(kk)
    if dtype is np.float32:                      # the f32 restatement adds the 64 products in the kernel's order, whatever the BLAS
        acc = np.zeros((L, H, len(rows), nF), np.float32)
        for e in range(64):
            acc += qw[..., e][..., None] * kk[:, :, e][:, :, None, :]
        return (acc * np.float32(0.125)).reshape(L * H, len(rows), nF)
    return ((qw @ kk) * dtype(0.125)).reshape(L * H, len(rows), nF)


def softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True, dtype=x.dtype)


def frame_filter(x, width, mode="reflect", fn=np.median):
    """whisper.timing.median_filter along the last axis (fn = np.max: the running maximum over the same windows)"""
    pad = width // 2
    if pad == 0 or x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode=mode)
    return fn(sliding_window_view(xp, width, axis=-1), axis=-1).astype(x.dtype)


def eps_p(case, Amax):
    """relative tolerance of a softmax probability whose logits carry the raw-score tolerance"""
    return (2.0 * C_RAW * Amax * case.opts["qk_scale"] + 24.0) * U32


def _order(score, largest):
    """head indices by score, the lowest head first on a tie (axis 0)"""
    return np.argsort(-score if largest else score, axis=0, kind="stable")


# ---------------------------------------------------------------------------------------------------------------- dynamic
def dynamic(case, q, k, dtype=np.float64, mutate=None):
    """per window: gathered [count][rows][F], dscore [LH][rows], sel [rows][count], matrix [rows][F] (+ the tolerances' magnitudes
    when dtype is float64 and nothing is mutated)"""
    assert case.kind == "dynamic" and (mutate is None or mutate in MUTATIONS["dynamic"])
    o, L, H, LH = case.opts, case.L, case.H, case.LH
    scale, count, width = dtype(o["qk_scale"]), o["count"], o["width"]
    out = {n: [] for n in QUANTITIES["dynamic"] + ("A_gathered", "Amax", "tol_matrix", "logits", "std", "pmin")}
    for w in range(case.W):
        F, nr = case.n_frames[w], case.rows(w)
        r0 = case.n_sot + (1 if mutate == "rows_plus_1" else -1 if mutate == "rows_minus_1" else 0)
        rows = np.arange(r0, r0 + nr)
        Fs = N_AUDIO_CTX if mutate == "softmax_all_frames" else F
        kw = (w - 1) % case.W if mutate == "k_of_previous_window" else None
        S = raw_scores(case, q, k, w, rows, Fs, dtype, kw)
        if mutate == "head_h_L_plus_l":
            S = np.ascontiguousarray(S.reshape(L, H, nr, Fs).transpose(1, 0, 2, 3)).reshape(LH, nr, Fs)
        z = S * (dtype(1.0) if mutate == "score_without_qk_scale" else scale)
        p = softmax(z)[..., :F]
        if o["peaks"] == "own":
            pk = F - 1 - np.argmax(z[..., :F][..., ::-1], axis=-1) if mutate == "peak_highest_on_tie" else np.argmax(z[..., :F], axis=-1)
            pk = pk.astype(dtype)
        else:
            pk = np.broadcast_to(case.peaks(w, mutate != "peaks_without_midpoint"), (LH, nr))       # f64, like the reference
        if mutate == "dist_from_peak_plus_1":
            pk = pk + 1
        dist = np.abs(pk[..., None] - np.arange(F, dtype=pk.dtype)) / pk.dtype.type(1500)
        score = (dist * p).sum(axis=-1).astype(np.float64)
        sel = _order(score, mutate == "largest_picks")[:count].T                                   # [rows][count]
        g = np.stack([S[sel[:, c], np.arange(nr), :F] for c in range(count)])                      # [count][rows][F]
        pz = softmax(g * scale)
        mu = pz.mean(axis=1, keepdims=True, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            sd = pz.std(axis=1, keepdims=True, dtype=np.float64, ddof=1 if mutate == "sample_std" else 0)
            zs = ((pz - mu.astype(dtype)) / sd.astype(dtype)).astype(dtype)
        med = frame_filter(zs, width)
        out["gathered"].append(g.astype(np.float64))
        out["dscore"].append(score)
        out["sel"].append(sel.astype(np.int32))
        out["matrix"].append((-(med.sum(axis=0, dtype=dtype) / dtype(count))).astype(np.float64) if case.matrix_compared(w) else None)
        if dtype is np.float64 and mutate is None:
            A = raw_scores(case, q, k, w, rows, F, absolute=True)
            Amax = A.max(axis=-1)
            Ag = np.stack([A[sel[:, c], np.arange(nr)] for c in range(count)])
            out["A_gathered"].append(Ag)
            out["Amax"].append(Amax)
            out["logits"].append(z)
            out["std"].append(sd)
            out["pmin"].append(min(p.min(), pz.min()))
            tm = None
            if case.matrix_compared(w):
                e = eps_p(case, Ag.max(axis=-1))[..., None] + 4 * U32                              # [count][rows][1]
                dp = e * pz
                dmu = dp.mean(axis=1, keepdims=True)
                dsd = dp.max(axis=1, keepdims=True) + dmu
                tz = (dp + dmu + np.abs(zs) * dsd) / sd + 4 * U32 * np.abs(zs)
                tm = frame_filter(tz, width, fn=np.max).mean(axis=0) + (count + 2) * U32 * np.abs(out["matrix"][-1]) + TINY
            out["tol_matrix"].append(tm)
    return out


# ---------------------------------------------------------------------------------------------------------------- new
def new_head_stats(case, q, k, w, dtype=np.float64, mutate=None, heads=None):
    """the per-head part of ``new`` for window w (heads: a subset, for the builder): p [heads][n][F], colnorm, score, tolerances"""
    o = case.opts
    scale, width = dtype(o["qk_scale"]), o["width"]
    F, n, r0 = case.n_frames[w], case.n_tok[w], case.n_sot
    nh = case.LH if heads is None else len(heads)
    if mutate == "crop_after_median":
        m = frame_filter(raw_scores(case, q, k, w, np.arange(n), N_AUDIO_CTX, dtype, heads=heads), width)[..., :F]
    else:
        S = raw_scores(case, q, k, w, np.arange(n), F, dtype, heads=heads)
        m = S if mutate == "median_after_softmax" else frame_filter(S, width, "symmetric" if mutate == "symmetric_padding" else "reflect")
    p = softmax(m * scale)
    if mutate == "median_after_softmax":
        p = frame_filter(p, width)
    cn = np.sqrt(((p[:, r0:n - 1] if mutate == "colnorm_text_rows" else p) ** 2).sum(axis=1, dtype=dtype))      # [heads][F]
    rn = (p ** 2).sum(axis=2, dtype=dtype)
    rn = rn if mutate == "rownorm_without_sqrt" else np.sqrt(rn)                                             # [heads][n]
    cov = p.sum(axis=1, dtype=dtype)
    pen_pos = (cov if mutate == "coverage_without_clamp" else np.maximum(cov, dtype(0.5))).sum(axis=-1, dtype=dtype)
    half = dtype(0.0 if mutate == "coverage_without_half_F" else 0.5 * F)
    score = np.zeros(nh, dtype)
    if o["w_col"] > 0:
        score += dtype(o["w_col"]) * cn.sum(axis=-1, dtype=dtype)
    if o["w_row"] > 0:
        score += dtype(o["w_row"]) * rn.sum(axis=-1, dtype=dtype)
    if o["w_cov"] > 0:
        score -= dtype(o["w_cov"]) * (pen_pos - half)
    st = dict(p=p, colnorm=cn, nscore=score.astype(np.float64), pmin=p.min())
    if dtype is np.float64 and mutate is None:
        e = eps_p(case, raw_scores(case, q, k, w, np.arange(n), F, absolute=True, heads=heads).max(axis=-1))   # [heads][n]
        e_cn = e.max(axis=1) + (n + 4) * U32
        mag, rounding = np.zeros(nh), 0.0
        if o["w_col"] > 0:
            mag += o["w_col"] * cn.sum(axis=-1)
        if o["w_row"] > 0:
            mag += o["w_row"] * rn.sum(axis=-1)
        if o["w_cov"] > 0:                       # the probabilities' error enters where the clamp lets it; the sum's rounding everywhere
            mag += o["w_cov"] * np.where(cov > 0.5, cov, 0.0).sum(axis=-1)
            rounding = 16 * U32 * o["w_cov"] * (pen_pos + 0.5 * F)
        st.update(eps=e, eps_cn=e_cn, tol_colnorm=e_cn[:, None] * cn + TINY,
                  tol_nscore=(e.max(axis=1) + (n + 24) * U32) * mag + rounding + TINY)
    return st


def new(case, q, k, dtype=np.float64, mutate=None):
    """per window: colnorm [LH][F], nscore [LH], top [topk], matrix [rows][F]"""
    assert case.kind == "new" and (mutate is None or mutate in MUTATIONS["new"])
    LH, topk, r0 = case.LH, case.opts["topk"], case.n_sot
    out = {n: [] for n in QUANTITIES["new"] + ("tol_colnorm", "tol_nscore", "tol_matrix", "pmin")}
    for w in range(case.W):
        st = new_head_stats(case, q, k, w, dtype, mutate)
        p, cn = st["p"], st["colnorm"]
        top = _order(st["nscore"], mutate != "smallest_picks")[:topk]
        lo = r0 + (1 if mutate == "out_rows_plus_1" else 0)
        terms = p[top, lo:lo + case.rows(w)] / cn[top][:, None, :]                                                  # [topk][rows][F]
        mat = -(terms.sum(axis=0, dtype=dtype) / dtype(LH if mutate == "mean_over_LH" else topk))
        out["colnorm"].append(cn.astype(np.float64))
        out["nscore"].append(st["nscore"])
        out["top"].append(top.astype(np.int32))
        out["matrix"].append(mat.astype(np.float64))
        out["pmin"].append(st["pmin"])
        if "eps" in st:
            out["tol_colnorm"].append(st["tol_colnorm"])
            out["tol_nscore"].append(st["tol_nscore"])
            et = st["eps"][top, r0:r0 + case.rows(w)][..., None] + st["eps_cn"][top][:, None, None] + (topk + 4) * U32
            out["tol_matrix"].append((terms * et).sum(axis=0) / topk + TINY)
    return out


def compute(case, q=None, k=None, dtype=np.float64, mutate=None):
    q = case.q if q is None else q
    k = case.k if k is None else k
    return (dynamic if case.kind == "dynamic" else new)(case, q, k, dtype, mutate)


def reference(case):
    """the float64 reference on the poisoned inputs"""
    ref = compute(case, *case.poisoned())
    for name in QUANTITIES[case.kind]:
        for x in ref[name]:
            assert x is None or np.isfinite(x).all(), (case.name, name)
    return ref


def pool(coefs, xs, dtype=np.float64):
    """sum_j c_j x_j and its tolerance magnitude sum_j |c_j x_j|"""
    terms = [np.asarray(c, dtype) * np.asarray(x, dtype) for c, x in zip(coefs, xs)]
    acc = np.zeros_like(terms[0])
    for t in terms:
        acc = acc + t
    return acc.astype(np.float64), np.sum([np.abs(t.astype(np.float64)) for t in terms], axis=0)


# ---------------------------------------------------------------------------------------------------------------- tolerances
def tol_gathered(case, ref, w):
    return C_RAW * U32 * ref["A_gathered"][w] + TINY


def tol_dscore(case, ref, w):
    return eps_p(case, ref["Amax"][w]) * ref["dscore"][w] + TINY


def tol_matrix(case, ref, w):
    return ref["tol_matrix"][w]


def tol_colnorm(case, ref, w):
    return ref["tol_colnorm"][w]


def tol_nscore(case, ref, w):
    return ref["tol_nscore"][w]


def tol_pool(n_in, mag):
    return 4 * n_in * U32 * mag + TINY


TOLERANCES = {"gathered": tol_gathered, "dscore": tol_dscore, "matrix": tol_matrix, "colnorm": tol_colnorm, "nscore": tol_nscore}
EXACT = ("sel", "top")


def ratio(got, ref, tol):
    """largest |got - ref| / tolerance; a NaN or infinity in `got` counts as infinitely far"""
    got = np.asarray(got, np.float64)
    r = np.abs(got - ref) / tol
    r[~np.isfinite(got)] = np.inf
    return float(r.max()) if r.size else 0.0


def worst_ratios(case, got, ref):
    """{quantity: worst ratio over the windows}; the picks compare exactly (0 or infinity)"""
    out = {}
    for name in QUANTITIES[case.kind]:
        worst = 0.0
        for w in range(case.W):
            if ref[name][w] is None:
                continue
            if name in EXACT:
                r = 0.0 if np.array_equal(np.asarray(got[name][w]), ref[name][w]) else np.inf
            else:
                r = ratio(got[name][w], ref[name][w], TOLERANCES[name](case, ref, w))
            worst = max(worst, r)
        out[name] = worst
    return out


# ---------------------------------------------------------------------------------------------------------------- conditions
def _tied_heads(case, a, b):
    return any({a, b} == {x, y} for x, y in case.ties.get("heads", ()))


def violations(case, ref):
    """[(what, w, head, row)]: the (window, head, row) entries that break a condition on the inputs (row None: the whole head)"""
    bad = []
    for w in range(case.W):
        if case.kind == "dynamic":
            nr, count = case.rows(w), case.opts["count"]
            if case.opts["peaks"] == "own" and case.n_frames[w] > 1:
                z = ref["logits"][w]
                top2 = np.partition(z, -2, axis=-1)[..., -2:]
                need = GAP * C_RAW * U32 * ref["Amax"][w] * case.opts["qk_scale"]
                for h, i in zip(*np.nonzero(top2[..., 1] - top2[..., 0] < need)):
                    tf = case.ties.get("frames")
                    if tf and tf[0] == w and top2[h, i, 1] == top2[h, i, 0] and z[h, i, tf[1]] == top2[h, i, 1] == z[h, i, tf[2]]:
                        continue
                    bad.append(("peak", w, int(h), int(i)))
            sc, tol = ref["dscore"][w], tol_dscore(case, ref, w)
            order = _order(sc, False)
            for r in range(min(count + 1, case.LH) - 1):
                a, b = order[r], order[r + 1]
                ii = np.arange(nr)
                close = sc[b, ii] - sc[a, ii] < GAP * np.maximum(tol[a, ii], tol[b, ii])
                for i in np.nonzero(close)[0]:
                    if not (_tied_heads(case, a[i], b[i]) and sc[a[i], i] == sc[b[i], i]):
                        bad.append(("order", w, int(b[i]), int(i)))
            if case.matrix_compared(w):             # ... and the rows of a column differ by more than their f32 rounding
                pz = softmax(ref["gathered"][w] * case.opts["qk_scale"])
                if not (ref["std"][w] >= np.maximum(1e-12, 8 * U32 * pz.max(axis=1, keepdims=True))).all():
                    bad.append(("std", w, -1, None))
        else:
            if w in case.ties.get("one_frame", ()):
                continue
            sc, tol = ref["nscore"][w], ref["tol_nscore"][w]
            order = _order(sc, True)
            for r in range(min(case.opts["topk"] + 1, case.LH) - 1):
                a, b = order[r], order[r + 1]
                if sc[a] - sc[b] < GAP * max(tol[a], tol[b]) and not (_tied_heads(case, a, b) and sc[a] == sc[b]):
                    bad.append(("order", w, int(b), None))
        if not ref["pmin"][w] >= 2.0 ** -126:
            bad.append(("subnormal", w, -1, None))
    return bad


# ---------------------------------------------------------------------------------------------------------------- builder
def _expected_frame(i, nr, F):
    return min(F - 1, int((i + 0.5) * F / nr))


def build_case(name, *, kind, f16, rows, frames, seed, wide=False, n_sot=3, frame_tie=False, twin_heads=False, xkv_W=0, window0=0,
               head_gains=(0.3, 2.2), **opts):
    """rows / frames: text rows and frames per window (n_tok = rows + n_sot + 1); frame_tie: two identical K rows under a planted
    peak of window 0; twin_heads (wide): heads WIDE_TWINS are copies of the two strongest planted heads below 256; xkv_W / window0:
    where the GPU test puts the windows inside a larger K buffer; opts: the call's options (module docstring).  The seeds in the
    case lists are the committed ones: the builder asserts the input conditions for them"""
    rng = np.random.default_rng(seed)
    L, H = (44, 6) if wide else (4, 6)
    LH, W, d = L * H, len(rows), 64 * H
    dt = np.float16 if f16 else np.float32
    n_tok = tuple(r + n_sot + 1 for r in rows)
    max_n = max(n_tok) + 1                                              # every window has at least one poisoned q row
    assert max_n <= 24 and W <= 3 and all(1 <= F <= N_AUDIO_CTX for F in frames)
    if kind == "dynamic":
        opts = dict(dict(count=4, width=7, qk_scale=1.0, peaks="own"), **opts)
    else:
        opts = dict(dict(topk=20, width=7, qk_scale=1.0, w_col=1.0, w_row=1.0, w_cov=0.0), **opts)
    k = rng.standard_normal((L, W, N_AUDIO_CTX, d), dtype=np.float32)
    q = np.zeros((L, W, max_n, d), np.float32)
    # planted heads: a few per window, on both sides of head 256 in the wide configuration; twins: copies of the two strongest
    planted, twins = [], []
    for w in range(W):
        if wide:
            heads = np.concatenate([rng.choice(250, 5, replace=False), rng.choice(WIDE_HIGH, 3, replace=False)])
        else:
            heads = rng.choice(LH, 6, replace=False)
        amps = rng.permutation(np.linspace(*((7.0, 11.0) if kind == "dynamic" else (4.5, 8.5)), len(heads)))
        planted.append({int(h): float(a) for h, a in zip(heads, amps)})
    if twin_heads:
        assert wide
        srcs = sorted((h for h in planted[0] if h < 250), key=lambda h: -planted[0][h])[:2]
        twins = list(zip(srcs, WIDE_TWINS))
        for w in range(W):                                              # the twins' sources are planted, and strongest, everywhere
            for (a, _), amp in zip(twins, (11.5, 11.25)):
                planted[w][a] = amp
    twin_of = {b: a for a, b in twins}
    tie = None
    if frame_tie:
        f1 = _expected_frame(0, rows[0], frames[0])
        tie = (0, f1, min(frames[0] - 1, f1 + 9))
        assert tie[2] > tie[1]
        k[:, 0, tie[2]] = k[:, 0, tie[1]]
    if kind == "new":
        # the median runs before the softmax and would remove a one-frame peak: the keys around every text row's expected frame
        # are near copies of that frame's, a plateau wider than any filter of the cases
        for w in range(W):
            for i in range(rows[w] if frames[w] >= 64 else 0):          # (a short window is all plateau: no head could be sharp)
                fi = _expected_frame(i, rows[w], frames[w])
                for f in range(max(0, fi - 7), min(frames[w], fi + 8)):
                    if f != fi:
                        k[:, w, f] = k[:, w, fi] + np.float32(0.05) * rng.standard_normal((L, d), dtype=np.float32)
    for a, b in twins:
        k[b // H, :, :, (b % H) * 64:(b % H + 1) * 64] = k[a // H, :, :, (a % H) * 64:(a % H + 1) * 64]
    k = k.astype(dt)
    k32 = k.astype(np.float32)

    # 'new' ranks whole heads: a gain per (window, head) on top of the rows' spreads the heads' sharpness, hence their scores
    head_gain = np.ones((W, LH))

    def new_head_gain(w, head):
        if kind == "new":
            head_gain[w, twin_of.get(head, head)] = np.exp(rng.uniform(np.log(head_gains[0]), np.log(head_gains[1])))

    def draw(w, head, i):
        """q of (window, head, row): random with a gain of its own, or aligned with a key near the row's expected frame (a few
        frames off, differently per head: with the previous pass's midpoints as peaks the planted heads' scores would coincide)"""
        head = twin_of.get(head, head)
        l, h = divmod(head, H)
        lo, hi = (0.5, 2.0) if kind == "dynamic" else (0.7, 1.4)
        v = rng.standard_normal(64).astype(np.float32) * np.float32(head_gain[w, head] * np.exp(rng.uniform(np.log(lo), np.log(hi))))
        nr = n_tok[w] - n_sot - 1
        if head in planted[w] and n_sot <= i < n_sot + nr:
            fi = _expected_frame(i - n_sot, nr, frames[w])
            if kind == "dynamic" and not (tie and (w, fi) == tie[:2]):
                fi = int(np.clip(fi + rng.integers(-6, 7), 0, frames[w] - 1))
            kf = k32[l, w, fi, h * 64:(h + 1) * 64]
            amp = (planted[w][head] + rng.uniform(-0.75, 0.75)) / opts["qk_scale"]       # (the SCALED peak logit is 7 .. 11)
            v = kf * np.float32(amp / (0.125 * float(kf @ kf))) + np.float32(0.3) * v / np.float32(max(1.0, np.abs(v).max() / 2))
        q[l, w, i, h * 64:(h + 1) * 64] = v
        for b, a in twin_of.items():
            if a == head:
                q[b // H, w, i, (b % H) * 64:(b % H + 1) * 64] = v

    for w in range(W):
        for head in range(LH):
            new_head_gain(w, head)
            for i in range(max_n):
                draw(w, head, i)
    ties = {}
    if tie:
        ties["frames"] = tie
    if twins:
        ties["heads"] = twins
    if kind == "new" and 1 in frames:
        ties["one_frame"] = [w for w, F in enumerate(frames) if F == 1]
    jumps = None
    if opts.get("peaks") == "mid":
        jumps = [np.array([i * F // r for i in range(r)]) for r, F in zip(rows, frames)]
    case = Case(name, kind, f16, L, H, n_sot, n_tok, tuple(frames), max_n, q.astype(dt), k, opts, jumps, planted, ties, xkv_W, window0)
    ref = compute(case)
    for _ in range(400):
        bad = violations(case, ref)
        if not bad:
            break
        for what, w, head, i in bad:
            assert what in ("peak", "order"), (name, what, w)            # the others are properties of the seed
            if i is None:
                new_head_gain(w, head)
            for row in ([i + n_sot] if i is not None else range(n_tok[w])):
                draw(w, head, row)
            case.redrawn += 1
        case.q = q.astype(dt)
        if kind == "dynamic":
            ref = compute(case)
        else:                                                            # only the redrawn heads' scores change
            for w in sorted({b[1] for b in bad}):
                hs = sorted({twin_of.get(b[2], b[2]) for b in bad if b[1] == w} | {t for b in bad if b[1] == w for t, a in twin_of.items()
                                                                                    if a == twin_of.get(b[2], b[2])})
                st = new_head_stats(case, case.q, case.k, w, heads=hs)
                ref["nscore"][w][hs], ref["tol_nscore"][w][hs] = st["nscore"], st["tol_nscore"]
                ref["pmin"][w] = min(ref["pmin"][w], st["pmin"])
    else:
        raise AssertionError((name, bad))
    return case


# ---------------------------------------------------------------------------------------------------------------- the case lists
def _both(name, **kw):
    for f16 in (False, True):
        yield f"{name}-{'f16' if f16 else 'f32'}", dict(kw, f16=f16)


def dynamic_cases():
    seed = 100
    for peaks in ("own", "mid"):
        for scale in (1.0, 2.0):
            seed += 1
            yield from _both(f"dyn-{peaks}-scale{scale:g}", kind="dynamic", rows=(2, 5, 12), frames=(4, 257, 1500), count=4, peaks=peaks,
                             width=7, qk_scale=scale, seed=seed)
    for width in (1, 3, 11):
        seed += 1
        yield from _both(f"dyn-width{width}", kind="dynamic", rows=(3, 3, 3), frames=(33, 255, 256), width=width, seed=seed)
    yield from _both("dyn-count1", kind="dynamic", rows=(2, 5), frames=(40, 301), count=1, seed=120)
    yield from _both("dyn-count24", kind="dynamic", rows=(2, 5), frames=(40, 301), count=24, seed=121)
    yield from _both("dyn-wide", kind="dynamic", wide=True, rows=(2, 3), frames=(987, 1499), count=6, twin_heads=True, seed=122)
    yield from _both("dyn-frame-tie", kind="dynamic", rows=(4, 3), frames=(200, 64), frame_tie=True, seed=123)
    yield from _both("dyn-subbatch", kind="dynamic", rows=(4, 7), frames=(130, 1000), peaks="mid", xkv_W=4, window0=1, seed=124)


def new_cases():
    yield from _both("new-short", kind="new", rows=(1, 5, 12), frames=(1, 3, 4), width=7, topk=1, seed=201)
    for cov in (0.0, 0.5):
        yield from _both(f"new-w11-cov{cov:g}", kind="new", rows=(2, 5, 12), frames=(6, 257, 1500), width=11, topk=7, w_cov=cov,
                         seed=202 + int(cov * 2))
    for width in (1, 5):
        yield from _both(f"new-width{width}", kind="new", rows=(3, 6), frames=(7, 987), width=width, topk=20, seed=210 + width)
    # width 13 (the rank-count median) over 7 frames returns the row's median, or a neighbour of it, at every frame: p is uniform
    # or nearly so for EVERY head whatever q and K are, and the scores of 24 heads lie within 8 % of each other -- less than 20
    # gaps of 100 tolerances.  So the order is asserted 20 deep on the long windows and 3 deep on the 7-frame window; column
    # norms, scores and the matrix are compared for all heads in both
    yield from _both("new-width13", kind="new", rows=(3, 6), frames=(40, 987), width=13, topk=20, seed=223)
    yield from _both("new-width13-short", kind="new", rows=(3, 6), frames=(7, 13), width=13, topk=3, seed=224)
    yield from _both("new-colnorm-only", kind="new", rows=(2, 6), frames=(50, 300), w_col=1.0, w_row=0.0, topk=5, seed=230)
    yield from _both("new-rownorm-only", kind="new", rows=(2, 6), frames=(50, 300), w_col=0.0, w_row=1.0, topk=5, seed=231)
    yield from _both("new-topk24", kind="new", rows=(2, 6), frames=(50, 300), topk=24, qk_scale=2.0, seed=232)
    yield from _both("new-wide", kind="new", wide=True, rows=(2, 3), frames=(130, 300), topk=20, twin_heads=True, seed=233)


def all_cases():
    yield from dynamic_cases()
    yield from new_cases()


def case_table(gen):
    return dict(gen)


_BUILT = {}


def get_case(name):
    """the case of that name, built once per process"""
    if name not in _BUILT:
        _BUILT[name] = build_case(name, **case_table(all_cases())[name])
    return _BUILT[name]


POOL_SIZES = (1, 255, 256, 40 * 1500 + 1)
POOL_N_IN = (1, 3, 8)


def pool_inputs(n_in, n, seed=7):
    rng = np.random.default_rng(seed + 1000 * n_in + n)
    xs = rng.standard_normal((n_in, n)).astype(np.float32)
    coef = rng.uniform(0.05, 1.0, n_in).astype(np.float32)
    return coef, xs
