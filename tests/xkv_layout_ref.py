"""The memory layouts between the encoder output and a decode step's cross-attention, stated on their own (numpy, no GPU).

Nothing here is transcribed from a kernel that WRITES these layouts (the GEMM epilogues, xkv_pack_kernel).  The fragment-ordered
("packed") copy is derived from what its CONSUMER says an MFMA operand register means:

  v_mfma_f32_16x16x32_f16 computes D[16][16] += A[16][32] B[32][16].  Lane l = 16 g + i (i = l & 15, g = l >> 4) holds, as its
  eight halfs e = 0..7, A[i][8 g + e] and B[8 g + e][i]; of D it holds D[4 g + r][i], r = 0..3.

  The decode cross-attention computes S^T = K Q^T per 32-key block as two 16-key tiles t = 0, 1 and wants lane (i, g) to end up with
  the probabilities of the eight CONSECUTIVE keys 8 g .. 8 g + 7 of the block (they are the B operand of O^T += V^T P^T, k index
  8 g + j <-> key 8 g + j).  D row 4 g + r of tile t therefore has to be key 8 g + 4 t + r, that is A row i of tile t is key
  (i >> 2) * 8 + (i & 3) + 4 t.  The 64 dims of a key are two k-steps kk = 0, 1 of 32: k index 8 g + e <-> dim 32 kk + 8 g + e.
     K fragment 2 t + kk, lane (i, g), half e  =  K[32 blk + (i >> 2) * 8 + (i & 3) + 4 t][32 kk + 8 g + e]
  O^T[64][16] is four 16-dim tiles t = 0..3 with A = V^T: A row i <-> dim 16 t + i, k index 8 g + e <-> key 8 g + e.
     V^T fragment t, lane (i, g), half e       =  V[32 blk + 8 g + e][16 t + i]
  A fragment is 64 lanes x 8 halfs = 512 halfs, a block 4 fragments; per head ceil(nk / 32) * 4 * 512 * 2 halfs, all K blocks first,
  then all V^T blocks; keys in [nk, ceil32(nk)) are zeros.
"""
import numpy as np

DH = 64


def ceil32(nk):
    return (nk + 31) // 32 * 32


def per_head(nk):
    """halfs of one head's fragment-ordered copy: K half, then V^T half"""
    return (nk + 31) // 32 * 4 * 512 * 2


def vt_index(b, h, dd, key, vt_kp, vt_bs):
    """element (batch item b, head h, dim dd, key) of the per-head transposed V, [B][H][64][vt_kp] with vt_bs elements between items"""
    return b * vt_bs + (h * DH + dd) * vt_kp + key


def cbatch_index(m, col, vt_s, vt_bs, ldc):
    """element (row m, column col) of a C whose rows are grouped in batch items of vt_s rows, vt_bs elements apart"""
    return (m // vt_s) * vt_bs + (m % vt_s) * ldc + col


def slot_map(nk):
    """For every slot of one head's packed array: (kind, key, dim) with kind 0 = K, 1 = V; key in [0, ceil32(nk))."""
    nblk = (nk + 31) // 32
    blk, f, g, i, e = np.meshgrid(np.arange(nblk), np.arange(4), np.arange(4), np.arange(16), np.arange(8), indexing="ij")
    # memory order inside a half: block, fragment, lane = 16 g + i, half e -- the axes above in this order
    t, kk = f >> 1, f & 1
    k_key = 32 * blk + (i >> 2) * 8 + (i & 3) + 4 * t
    k_dim = 32 * kk + 8 * g + e
    v_key = 32 * blk + 8 * g + e
    v_dim = 16 * f + i
    n = k_key.size
    kind = np.concatenate([np.zeros(n, np.int64), np.ones(n, np.int64)])
    key = np.concatenate([k_key.ravel(), v_key.ravel()])
    dim = np.concatenate([k_dim.ravel(), v_dim.ravel()])
    assert kind.size == per_head(nk)
    return kind, key, dim


def packed_from(K, V, nk):
    """K, V [nk][H * 64] -> [H][per_head(nk)] of the same dtype."""
    K, V = np.asarray(K), np.asarray(V)
    assert K.shape == V.shape and K.shape[0] == nk and K.shape[1] % DH == 0
    H = K.shape[1] // DH
    kind, key, dim = slot_map(nk)
    n32 = ceil32(nk)
    out = np.zeros((H, kind.size), K.dtype)
    for h in range(H):
        src = np.zeros((2, n32, DH), K.dtype)
        src[0, :nk] = K[:, h * DH:(h + 1) * DH]
        src[1, :nk] = V[:, h * DH:(h + 1) * DH]
        out[h] = src[kind, key, dim]
    return out


def unpack(P, nk):
    """inverse of packed_from: [H][per_head(nk)] -> K, V [nk][H * 64] and the values found in the padding slots"""
    P = np.asarray(P)
    H = P.shape[0]
    kind, key, dim = slot_map(nk)
    assert P.shape[1] == kind.size
    n32 = ceil32(nk)
    K = np.zeros((nk, H * DH), P.dtype)
    V = np.zeros((nk, H * DH), P.dtype)
    for h in range(H):
        src = np.zeros((2, n32, DH), P.dtype)
        src[kind, key, dim] = P[h]
        K[:, h * DH:(h + 1) * DH] = src[0, :nk]
        V[:, h * DH:(h + 1) * DH] = src[1, :nk]
    pad = P[:, key >= nk]
    return K, V, pad


def attention_from_packed(q, P, nk):
    """softmax(q K^T / 8) V in float64, read from the packed array one 32-key block at a time through the operand meaning above:
    q [nq][H * 64], P [H][per_head(nk)] -> [nq][H * 64]"""
    q = np.asarray(q, np.float64)
    P = np.asarray(P, np.float64)
    H = P.shape[0]
    nq = q.shape[0]
    nblk = (nk + 31) // 32
    half = per_head(nk) // 2
    out = np.zeros((nq, H * DH))
    for h in range(H):
        qh = q[:, h * DH:(h + 1) * DH]
        kf = P[h, :half].reshape(nblk, 4, 4, 16, 8)            # [blk][fragment][g][i][e]
        vf = P[h, half:].reshape(nblk, 4, 4, 16, 8)
        s = np.full((nq, nblk * 32), -np.inf)
        for blk in range(nblk):
            for t in range(2):
                a = np.zeros((16, DH))                          # the A operand rows of tile t over both k-steps: [i][dim]
                for kk in range(2):
                    for g in range(4):
                        a[:, 32 * kk + 8 * g:32 * kk + 8 * g + 8] = kf[blk, 2 * t + kk, g]
                st = a @ qh.T * 0.125                           # D[row][query]; row 4 g + r is key 8 g + 4 t + r of the block
                for row in range(16):
                    key = 32 * blk + (row >> 2) * 8 + 4 * t + (row & 3)
                    if key < nk:
                        s[:, key] = st[row]
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        o = np.zeros((DH, nq))
        for blk in range(nblk):
            pb = p[:, 32 * blk:32 * blk + 32].T                 # B operand: k index = key within the block
            for t in range(4):
                a = np.zeros((16, 32))                          # [i = dim 16 t + i][k = key 8 g + e]
                for g in range(4):
                    a[:, 8 * g:8 * g + 8] = vf[blk, t, g]
                o[16 * t:16 * t + 16] += a @ pb
        out[:, h * DH:(h + 1) * DH] = o.T
    return out


def attention_f64(q, K, V):
    """plain softmax(q K^T / 8) V per head in float64: q [nq][H * 64], K, V [nk][H * 64]"""
    q, K, V = (np.asarray(x, np.float64) for x in (q, K, V))
    H = q.shape[1] // DH
    out = np.zeros_like(q)
    for h in range(H):
        sl = slice(h * DH, (h + 1) * DH)
        s = q[:, sl] @ K[:, sl].T * 0.125
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        out[:, sl] = p @ V[:, sl]
    return out
