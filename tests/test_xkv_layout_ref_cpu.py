"""tests/xkv_layout_ref.py against itself and against plain float64 attention (no GPU): the fragment-ordered cross-K/V layout is a
bijection, its halves do not overlap, its padding is zero, it inverts, and attention evaluated from it block by block through the
MFMA operand meaning is attention.  The GPU tests (test_gpu_gemm_layout.py, test_gpu_xattn_packed.py) hold the kernels to this file."""
import numpy as np
import pytest

import xkv_layout_ref as xr

NKS = [128, 132, 156, 160, 1500]


@pytest.mark.parametrize("nk", NKS)
def test_slot_map_is_a_bijection_with_disjoint_halves(nk):
    kind, key, dim = xr.slot_map(nk)
    n = xr.per_head(nk)
    n32 = xr.ceil32(nk)
    assert n == (nk + 31) // 32 * 4 * 512 * 2 == 2 * n32 * 64 and kind.size == n
    # K half first, V^T half second: the two halves are the two kinds, nothing else
    assert (kind[:n // 2] == 0).all() and (kind[n // 2:] == 1).all()
    assert key.min() == 0 and key.max() == n32 - 1 and dim.min() == 0 and dim.max() == 63
    # every (kind, key, dim) of the padded problem exactly once  <=>  the map onto [0, per_head) is one to one and onto
    code = (kind * n32 + key) * 64 + dim
    assert np.array_equal(np.sort(code), np.arange(n))
    # a 16-byte piece (8 halfs) is 8 dims of one key (K) or 8 keys of one dim (V^T): what one lane loads
    c8 = code.reshape(-1, 8)
    assert (np.diff(c8[:n // 16], axis=1) == 1).all() and (np.diff(c8[n // 16:], axis=1) == 64).all()


@pytest.mark.parametrize("nk", NKS)
@pytest.mark.parametrize("H", [1, 3])
def test_packed_from_pads_with_zeros_and_inverts(nk, H):
    rng = np.random.default_rng(nk + H)
    K = rng.standard_normal((nk, H * 64)).astype(np.float16)
    V = rng.standard_normal((nk, H * 64)).astype(np.float16)
    K[K == 0] = 1
    V[V == 0] = 1                                              # no zero in the data: every zero of the result is padding
    P = xr.packed_from(K, V, nk)
    assert P.shape == (H, xr.per_head(nk)) and P.dtype == np.float16
    _, key, _ = xr.slot_map(nk)
    assert (P[:, key >= nk] == 0).all() and (P[:, key < nk] != 0).all()
    assert (key >= nk).sum() == 2 * 64 * (xr.ceil32(nk) - nk)
    K2, V2, pad = xr.unpack(P, nk)
    assert np.array_equal(K2.view(np.uint16), K.view(np.uint16)) and np.array_equal(V2.view(np.uint16), V.view(np.uint16))
    assert pad.size == H * 2 * 64 * (xr.ceil32(nk) - nk) and (pad == 0).all()


@pytest.mark.parametrize("nk", NKS)
def test_attention_from_the_packed_array_is_attention(nk):
    # ties the layout to the operation: K and V asymmetric random, queries scaled so that the softmax is neither flat nor one-hot
    rng = np.random.default_rng(7 * nk)
    H, nq = 2, 5
    q = rng.standard_normal((nq, H * 64)) * 1.5
    K = rng.standard_normal((nk, H * 64))
    V = rng.standard_normal((nk, H * 64)) + np.arange(H * 64) * 0.01
    got = xr.attention_from_packed(q, xr.packed_from(K, V, nk), nk)
    ref = xr.attention_f64(q, K, V)
    assert np.abs(got - ref).max() < 1e-12


def test_a_wrong_operand_meaning_is_not_attention():
    # the control of the test above: the same evaluation on an array packed with K's two 16-key tiles swapped is off by O(1)
    nk, H = 132, 1
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, 64)) * 1.5
    K = rng.standard_normal((nk, 64))
    V = rng.standard_normal((nk, 64))
    P = xr.packed_from(K, V, nk)
    half = xr.per_head(nk) // 2
    Pk = P[:, :half].reshape(H, -1, 4, 512).copy()
    Pk[:, :, [0, 1, 2, 3]] = Pk[:, :, [2, 3, 0, 1]]
    P2 = P.copy()
    P2[:, :half] = Pk.reshape(H, half)
    assert np.abs(xr.attention_from_packed(q, P2, nk) - xr.attention_f64(q, K, V)).max() > 1e-2


def test_vt_and_cbatch_index():
    B, H, vt_s, vt_kp, ldc = 3, 2, 132, 160, 128
    vt_bs = vt_s * ldc + H * 64 * vt_kp + 24
    seen = set()
    for b in range(B):
        for h in range(H):
            for dd in (0, 1, 63):
                for key in (0, 1, vt_s - 1, vt_kp - 1):
                    seen.add(xr.vt_index(b, h, dd, key, vt_kp, vt_bs))
    assert len(seen) == B * H * 3 * 4
    assert xr.vt_index(1, 1, 2, 3, vt_kp, vt_bs) == vt_bs + (64 + 2) * vt_kp + 3
    assert xr.cbatch_index(0, 5, vt_s, vt_bs, ldc) == 5
    assert xr.cbatch_index(vt_s - 1, 0, vt_s, vt_bs, ldc) == (vt_s - 1) * ldc
    assert xr.cbatch_index(vt_s, 7, vt_s, vt_bs, ldc) == vt_bs + 7
    assert xr.cbatch_index(2 * vt_s + 3, 127, vt_s, vt_bs, ldc) == 2 * vt_bs + 3 * ldc + 127
