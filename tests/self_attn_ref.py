"""Float64 statement of the decoder's cached self-attention (csrc/swx_selfattn.hip: self_attn_cached, kv_append_kernel,
self_attn_cached_mq_f16, self_attn_step_f16, self_attn_step_long_f16) and the inputs its tests run on.  No GPU, no library.

Contract.  Grid row ``ri`` is logical row ``r = ri * row_mul``; token ``i`` of it sits at position ``pos = pos0[r] + i``.  For
head ``h`` it attends to the keys ``j = 0 .. pos``; key ``j`` is read from cache row ``anc[r][j]`` when an ancestor table is
given, else from row ``r``; score ``q . k * 0.125``, softmax over ``j``, output ``sum_j p_j v_j``.  With ``skip_append == 0``
K / V of the new tokens (columns ``d .. 3d`` of the qkv rows) are first copied to position ``pos0[r] + i`` of row ``r``; nothing
else in the caches changes.  The single-token step kernels take the newest position from row ``r`` itself whatever the table
says there, so the builder sets ``anc[r][pos0[r] .. pos0[r] + n_new) = r`` -- what the beam update writes.

Inputs.  Every cache entry that no ``(row, j <= pos)`` references is NaN, except position 0 of the logical rows (the clamped
loads of lanes past ``pos`` read it and must discard it): a kernel that reads one position too far, or the wrong row, returns NaN
or a large error instead of what a sibling kernel with the same mistake would return.

Tolerance, elementwise: ``|got - ref| <= u |ref| + 2e-5 A + 1e-7`` with ``u = 2^-11`` (f16 output: half an ulp of the one
rounding) or ``2^-24`` (f32) and ``A = sum_j p_j |v_j|`` in float64; the ``2e-5 A`` term covers the f32 accumulation of the
scores and expf (tests/test_self_attn_ref_cpu.py measures an f32 restatement against it).
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

N_CTX = 448
STEP_POSITIONS = (0, 1, 7, 8, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 446, 447)
STEP_POSITIONS_SHORT = tuple(p for p in STEP_POSITIONS if p <= 127)
RAGGED_POS0 = (0, 3, 60, 120, 440)
MULTI_N_NEW = (1, 7, 8, 9, 31, 32, 33, 200, 448)     # 200: the first staged length (a multiple of 8) at which MQ8 asks for more than 64 KB of LDS
MUTATIONS = ("drop_newest", "wrong_ancestor", "head_off_by_one", "scale_0.124", "swap_v")

# kernel ids of swx_test_self_attn_plan (csrc/swx_kernels.h::SwxSelfAttnKernel)
K_CACHED_F16, K_CACHED_F32, K_MQ4, K_MQ8, K_STEP, K_STEP_WG5, K_STEP_LONG, K_STEP_LONG_WG5, K_STEP_DEEP = range(9)
KERNEL_NAMES = ("self_attn_cached<f16>", "self_attn_cached<float>", "self_attn_cached_mq_f16<4>", "self_attn_cached_mq_f16<8>",
                "self_attn_step_f16<false,1>", "self_attn_step_f16<false,5>", "self_attn_step_f16<true,1>",
                "self_attn_step_f16<true,5>", "self_attn_step_long_f16")
FLAG_NO_DEEP, FLAG_WG5 = 4, 134217728


@dataclass
class Case:
    name: str
    f16: bool
    R: int                      # grid rows
    row_mul: int
    H: int
    n_new: int
    n_ctx: int
    skip_append: bool
    q: np.ndarray               # [R * n_new][d], storage precision
    k_new: np.ndarray           # [R * n_new][d] K / V of the new tokens
    v_new: np.ndarray
    pos0: np.ndarray            # int32 [R * row_mul]
    anc: Optional[np.ndarray]   # int32 [R * row_mul][n_ctx] or None
    kc_dense: np.ndarray        # [R * row_mul][n_ctx][d] caches AFTER the append, every entry finite (the mutation checks read these)
    vc_dense: np.ndarray
    referenced: np.ndarray      # bool [R * row_mul][n_ctx]: some (row, j <= pos) reads this entry
    appended: np.ndarray        # bool [R * row_mul][n_ctx]: a new token's position

    @property
    def d(self):
        return 64 * self.H

    @property
    def rows_phys(self):
        return self.R * self.row_mul

    @property
    def dtype(self):
        return np.float16 if self.f16 else np.float32

    @property
    def u(self):
        return 2.0 ** -11 if self.f16 else 2.0 ** -24

    def _poisoned(self, dense, before):
        keep = self.referenced.copy()
        keep[np.arange(self.R) * self.row_mul, 0] = True
        out = dense.copy()
        out[~keep] = np.nan
        if before and not self.skip_append:
            out[self.appended] = np.nan          # the launch writes these
        return out

    def caches_before(self):
        """what the launch is given: unreferenced entries NaN; when the launch appends, the new tokens' entries NaN too"""
        return self._poisoned(self.kc_dense, True), self._poisoned(self.vc_dense, True)

    def caches_after(self):
        """what the caches must hold afterwards, bit for bit (NaN where they were NaN)"""
        return self._poisoned(self.kc_dense, False), self._poisoned(self.vc_dense, False)

    def qkv(self):
        """the launch's qkv rows: q alone (row stride d) when the new K / V are in the cache already, else q | k | v (stride 3d)"""
        if self.skip_append:
            return self.q.copy()
        return np.concatenate([self.q, self.k_new, self.v_new], axis=1)


def build_case(name, *, f16, H, n_new, pos0, q_scale, use_anc, row_mul=1, skip_append=True, n_ctx=N_CTX, seed=0):
    """pos0: position of the first new token of every grid row.  Ancestors of the older positions are drawn within groups of five
    cache rows (the beams of a window); with row_mul = 5 that is the group of the logical row"""
    rng = np.random.default_rng(seed)
    R, d = len(pos0), 64 * H
    Rp = R * row_mul
    dt = np.float16 if f16 else np.float32
    q = (rng.standard_normal((R * n_new, d)) * q_scale).astype(dt)
    k_new = (rng.standard_normal((R * n_new, d)) * 0.8).astype(dt)
    v_new = rng.standard_normal((R * n_new, d)).astype(dt)
    kc = (rng.standard_normal((Rp, n_ctx, d), dtype=np.float32) * np.float32(0.8)).astype(dt)
    vc = rng.standard_normal((Rp, n_ctx, d), dtype=np.float32).astype(dt)
    p0 = np.full(Rp, 77, np.int32)              # entries of rows that are no grid row: valid, and different from their neighbours'
    p0[::row_mul] = np.asarray(pos0, np.int32)
    assert (p0[::row_mul] + n_new <= n_ctx).all()
    anc = None
    if use_anc:
        grp = (np.arange(Rp) // 5 * 5)[:, None]
        anc = np.minimum(grp + rng.integers(0, 5, (Rp, n_ctx)), Rp - 1).astype(np.int32)
    referenced = np.zeros((Rp, n_ctx), bool)
    appended = np.zeros((Rp, n_ctx), bool)
    for ri in range(R):
        r = ri * row_mul
        lo, hi = int(p0[r]), int(p0[r]) + n_new
        if anc is not None:
            anc[r, lo:hi] = r
        appended[r, lo:hi] = True
        kc[r, lo:hi] = k_new[ri * n_new:(ri + 1) * n_new]
        vc[r, lo:hi] = v_new[ri * n_new:(ri + 1) * n_new]
    for ri in range(R):
        r = ri * row_mul
        j = np.arange(int(p0[r]) + n_new)
        referenced[anc[r, j] if anc is not None else r, j] = True
    return Case(name, f16, R, row_mul, H, n_new, n_ctx, skip_append, q, k_new, v_new, p0, anc, kc, vc, referenced, appended)


def _mutation_row(case):
    """the grid row the single-entry mutations act on: the one with the most keys (its probabilities are the smallest)"""
    return int(np.argmax(case.pos0[::case.row_mul]))


def attention(case, kc, vc, dtype=np.float64, mutate=None):
    """(out, A): out [R * n_new][d] and A = sum_j p_j |v_j| of the same shape, computed in `dtype` from caches kc / vc (after the
    append).  mutate: one of MUTATIONS -- a deliberately wrong statement (tests/test_self_attn_ref_cpu.py)"""
    assert mutate is None or mutate in MUTATIONS
    H, n_new, d = case.H, case.n_new, case.d
    out = np.zeros((case.R * n_new, d), dtype)
    A = np.zeros((case.R * n_new, d), dtype)
    scale = dtype(0.124 if mutate == "scale_0.124" else 0.125)
    mrow = _mutation_row(case)
    for ri in range(case.R):
        r = ri * case.row_mul
        p0 = int(case.pos0[r])
        n = p0 + n_new
        j = np.arange(n)
        rows = case.anc[r, :n].copy() if case.anc is not None else np.full(n, r)
        if mutate == "wrong_ancestor" and ri == mrow:
            jm = (n - 1) // 2                   # one older position read from another row of the group
            g0 = r // 5 * 5
            others = [x for x in range(g0, min(g0 + 5, case.rows_phys)) if x != rows[jm]]
            if not others:                      # (a single cache row: no other row to read)
                others = [rows[jm]]
            rows[jm] = others[(jm + r) % len(others)]
        K = kc[rows, j].astype(dtype).reshape(n, H, 64)
        V = vc[rows, j].astype(dtype).reshape(n, H, 64)
        if mutate == "head_off_by_one":
            K, V = np.roll(K, -1, axis=1), np.roll(V, -1, axis=1)
        if mutate == "swap_v" and ri == mrow and n >= 2:
            ja, jb = (n - 1) // 3, n - 1
            V = V.copy()
            V[[ja, jb]] = V[[jb, ja]]
        Q = case.q[ri * n_new:(ri + 1) * n_new].astype(dtype).reshape(n_new, H, 64)
        Qh, Kh, Vh = Q.transpose(1, 0, 2), K.transpose(1, 0, 2), V.transpose(1, 0, 2)      # [H][tokens or keys][64]
        s = (Qh @ Kh.transpose(0, 2, 1)) * scale                       # [H][n_new][n]
        pos = p0 + np.arange(n_new)
        live = j[None, :] < pos[:, None] if mutate == "drop_newest" else j[None, :] <= pos[:, None]
        s = np.where(live[None], s, -np.inf)
        with np.errstate(invalid="ignore"):                            # (drop_newest at position 0: no key at all -> NaN)
            e = np.exp(s - s.max(axis=2, keepdims=True))
            p = (e / e.sum(axis=2, keepdims=True)).astype(dtype)
        # (a masked key's probability is exactly zero, but every key gathered here is one the contract reads: no NaN meets it)
        o = (p @ Vh).transpose(1, 0, 2)
        out[ri * n_new:(ri + 1) * n_new] = o.reshape(n_new, d)
        A[ri * n_new:(ri + 1) * n_new] = (p @ np.abs(Vh)).transpose(1, 0, 2).reshape(n_new, d)
    return out, A


def reference(case):
    """the float64 reference on the caches the launch leaves behind (NaN where the contract reads nothing): (out, A)"""
    kc, vc = case.caches_after()
    out, A = attention(case, kc, vc)
    assert np.isfinite(out).all(), case.name
    return out, A


def tolerance(case, ref, A):
    return case.u * np.abs(ref) + 2e-5 * A + 1e-7


def worst_ratio(case, got, ref, A):
    """largest |got - ref| / tolerance over the elements; a NaN or infinity in `got` counts as infinitely far"""
    got = np.asarray(got, np.float64)
    ratio = np.abs(got - ref) / tolerance(case, ref, A)
    ratio[~np.isfinite(got)] = np.inf
    return float(ratio.max())


def same_bits(a, b):
    """equal bit patterns (NaN entries included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    it = np.uint16 if a.dtype == np.float16 else np.uint32
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(it), b.view(it))


# ------------------------------------------------------------------------------------------------------ the case lists
GEOMETRIES = [(H, qs) for H in (2, 6) for qs in (0.8, 3.0)]


def step_cases(short):
    """single-token step: one launch with a row at every boundary position (short: the positions <= 127 only)"""
    positions = STEP_POSITIONS_SHORT if short else STEP_POSITIONS
    for H, qs in GEOMETRIES:
        for use_anc in (False, True):
            name = f"step-{'short' if short else 'all'}-H{H}-q{qs}-{'anc' if use_anc else 'noanc'}"
            yield name, dict(f16=True, H=H, n_new=1, pos0=positions, q_scale=qs, use_anc=use_anc,
                             seed=1000 + 100 * H + int(qs * 10) + 2 * use_anc + short)


def multi_cases():
    """multi-token pass, every row from position 0, no table"""
    for H, qs in GEOMETRIES:
        for R in (1, 3):
            for n_new in MULTI_N_NEW:
                yield f"multi-H{H}-q{qs}-R{R}-n{n_new}", dict(f16=True, H=H, n_new=n_new, pos0=(0,) * R, q_scale=qs, use_anc=False,
                                                             seed=2000 + 1000 * H + int(qs * 10) + 100 * R + n_new)


def general_cases():
    """general path: append then attend, q | k | v rows, ragged start positions, both dtypes, row_mul 1 and 5"""
    for f16 in (True, False):
        for H, qs in GEOMETRIES:
            for row_mul in (1, 5):
                for n_new in (1, 4, 8):
                    for use_anc in (False, True):
                        name = f"general-{'f16' if f16 else 'f32'}-H{H}-q{qs}-mul{row_mul}-n{n_new}-{'anc' if use_anc else 'noanc'}"
                        yield name, dict(f16=f16, H=H, n_new=n_new, pos0=RAGGED_POS0, q_scale=qs, use_anc=use_anc, row_mul=row_mul,
                                         skip_append=False, seed=3000 + 500 * f16 + 100 * H + int(qs * 10) + 7 * row_mul + 2 * n_new + use_anc)


def all_cases():
    for short in (False, True):
        yield from step_cases(short)
    yield from multi_cases()
    yield from general_cases()


def case_table(gen):
    """{name: kwargs} of a case generator, for pytest.mark.parametrize"""
    return dict(gen)
