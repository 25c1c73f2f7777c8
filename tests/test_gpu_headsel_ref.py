"""The head-selection kernels (csrc/swx_headsel.hip: headsel_score / headsel_pick / headsel_gather, newal_head / newal_pick /
newal_mean, weighted_sum) and the z-normalisation that follows the gather (csrc/swx_align.hip) against the float64 contract of
tests/headsel_ref.py.

Until this file the stage was compared with itself (the batch calls with the single-window calls: tests/test_gpu_headsel_batch.py)
and, loosely, with one reference run of tiny.en.  Here the C entries run on captured queries and cross-K built by hand -- no
network pass, a weightless handle -- in f32 and f16, on tiny's decoder shape (24 heads) and on a 44-layer one (264 heads: the
second trip of the pick kernels' 256-thread stride).  Everything the contract does not read is NaN: q rows past a window's
tokens, K rows past its frames, the V^T and packed parts of every K chunk, the chunks outside a sub-batch, the padding of the
peaks.  Every intermediate the kernels keep is read back through swx_test_heads_layout and compared with its own tolerance:
gathered raw rows, head scores, picks (exactly, in order), column norms, 'new' scores; then the matrix, which must be within
tolerance where the contract writes and bit-untouched elsewhere.  Tolerances, input conditions and the wrong statements they
reject: tests/headsel_ref.py, tests/test_headsel_ref_cpu.py.
"""
import ctypes

import numpy as np
import pytest
import torch

import headsel_ref as hr

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: "never written"
DYNAMIC = hr.case_table(hr.dynamic_cases())
NEW = hr.case_table(hr.new_cases())
_HANDLES = {}


def _lib():
    from stable_ts_amd import _lib
    return _lib.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _i32(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


def _handle(case):
    """a weightless handle per (decoder shape, dtype), made once: swx_heads_* only need the dims and a bound arena"""
    key = (case.L, case.H, case.f16)
    if key not in _HANDLES:
        from stable_ts_amd._lib import swx_dims
        lib = _lib()
        dims = swx_dims(n_mels=80, n_audio_ctx=hr.N_AUDIO_CTX, n_audio_state=384, n_audio_head=6, n_audio_layer=4, n_vocab=51865,
                        n_text_ctx=448, n_text_state=case.d, n_text_head=case.H, n_text_layer=case.L)
        h = ctypes.c_void_p()
        assert lib.swx_model_create(ctypes.byref(dims), 1 if case.f16 else 0, ctypes.byref(h)) == 0
        arena = torch.empty(lib.swx_weights_bytes(h), dtype=torch.uint8, device="cuda")
        assert lib.swx_bind_weights(h, _p(arena), arena.numel()) == 0
        _HANDLES[key] = (h, arena)
    return _HANDLES[key][0]


def _layout(lib, h, W, max_n, count):
    out = (ctypes.c_int64 * 9)()
    assert lib.swx_test_heads_layout(h, W, max_n, count, out) == 0
    return dict(zip(("cnt", "score", "sel", "colnorm", "nscore", "top", "gathered", "rstat", "total"), out))


def _region(scratch, off, dtype, shape):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return scratch[off:off + n].view(dtype).view(*shape).cpu().numpy()


def _nan_filled(*shape):
    out = torch.empty(*shape, dtype=torch.float32, device="cuda")
    out.view(torch.int32).fill_(NAN_BITS)
    return out


def _device_inputs(lib, h, case, windows=None, xkv_W=None, window0=0):
    """(q, xkv buffer, pointer to the first window's chunk): q [L][W][max_n][d] poisoned; K chunks of `windows` at window0 .. of a
    buffer of xkv_W windows that is NaN everywhere else"""
    qp, kp = case.poisoned()
    windows = list(range(case.W)) if windows is None else windows
    W = len(windows)
    xkv_W = xkv_W or W
    tdt = torch.float16 if case.f16 else torch.float32
    chunk_bytes = lib.swx_cross_kv_bytes(h, 1) // case.L
    chunk = chunk_bytes // (2 if case.f16 else 4)
    assert chunk >= hr.N_AUDIO_CTX * case.d
    xkv = torch.full((case.L, xkv_W, chunk), float("nan"), dtype=tdt, device="cuda")
    k = torch.from_numpy(np.ascontiguousarray(kp[:, windows])).cuda()
    xkv[:, window0:window0 + W, :hr.N_AUDIO_CTX * case.d] = k.view(case.L, W, -1)
    q = torch.from_numpy(np.ascontiguousarray(qp[:, windows])).cuda()
    return q, xkv, ctypes.c_void_p(xkv.data_ptr() + window0 * chunk_bytes)


def _report(case, got, ref, what):
    ratios = hr.worst_ratios(case, got, ref)
    print(f"headsel ratio case={case.name} call={what} " + " ".join(f"{k}={v:.4f}" for k, v in ratios.items()))
    for quantity, r in ratios.items():
        assert r <= 1.0, (case.name, what, quantity, r)


def _check_matrix_block(case, out, what):
    """the call wrote rows < n_rows[w], frames < F[w] of every window and nothing else; no NaN where the contract is defined"""
    bits = out.view(torch.int32).cpu().numpy()
    vals = out.cpu().numpy()
    untouched = np.ones(bits.shape, bool)
    mats = []
    for w in range(case.W):
        nr, F = case.rows(w), case.n_frames[w]
        untouched[w, :nr, :F] = False
        mats.append(vals[w, :nr, :F].astype(np.float64))
        if case.matrix_compared(w):
            assert np.isfinite(mats[-1]).all(), (case.name, what, w)
    assert (bits[untouched] == np.int32(NAN_BITS)).all(), (case.name, what, "wrote outside its block")
    return mats


# ---------------------------------------------------------------------------------------------------------------- dynamic
def _peaks(case, windows, R):
    if case.jumps is None:
        return None
    pk = np.full((len(windows), R), np.nan)
    for k, w in enumerate(windows):
        pk[k, :case.rows(w)] = case.peaks(w)
    return torch.from_numpy(pk).cuda()


def _run_dynamic_batch(lib, case, width=None):
    h = _handle(case)
    o = case.opts
    q, xkv, xkv_ptr = _device_inputs(lib, h, case, xkv_W=case.xkv_W, window0=case.window0)
    W, R, count = case.W, case.max_rows, o["count"]
    lay = _layout(lib, h, W, case.max_n, count)
    scratch = torch.full((lay["total"],), 0xFF, dtype=torch.uint8, device="cuda")
    peaks = _peaks(case, range(W), R)
    out = _nan_filled(W, R, hr.N_AUDIO_CTX)
    rc = lib.swx_heads_dynamic_batch(h, _p(q), W, case.max_n, case.n_sot, _i32(case.n_tok), _i32(case.n_frames), xkv_ptr, case.xkv_W,
                                     o["qk_scale"], o["width"] if width is None else width, count, _p(peaks), _p(out), hr.N_AUDIO_CTX,
                                     _p(scratch), scratch.numel(), _stream())
    torch.cuda.synchronize()
    return rc, out, scratch, lay


@pytest.mark.parametrize("name", list(DYNAMIC))
def test_dynamic_batch_against_f64(name):
    lib = _lib()
    case = hr.get_case(name)
    ref = hr.reference(case)
    rc, out, scratch, lay = _run_dynamic_batch(lib, case)
    assert rc == 0
    W, R, LH, count = case.W, case.max_rows, case.LH, case.opts["count"]
    score = _region(scratch, lay["score"], torch.float64, (W, LH, R))
    sel = _region(scratch, lay["sel"], torch.int32, (W, R, count))
    gathered = _region(scratch, lay["gathered"], torch.float32, (W, count, R, hr.N_AUDIO_CTX))
    cnt = _region(scratch, lay["cnt"], torch.int32, (3, W))
    assert cnt.tolist() == [list(case.n_tok), [case.rows(w) for w in range(W)], list(case.n_frames)]
    got = dict(dscore=[score[w, :, :case.rows(w)] for w in range(W)], sel=[sel[w, :case.rows(w)] for w in range(W)],
               gathered=[gathered[w, :, :case.rows(w), :case.n_frames[w]] for w in range(W)],
               matrix=_check_matrix_block(case, out, "batch"))
    _report(case, got, ref, "batch")


@pytest.mark.parametrize("name", [n for n in DYNAMIC if n.startswith(("dyn-own-scale", "dyn-mid-scale"))])
def test_dynamic_single_window_entries_against_f64(name):
    """swx_heads_dynamic + swx_align_weights, one window at a time, on the first row of the case table"""
    lib = _lib()
    case = hr.get_case(name)
    ref = hr.reference(case)
    h = _handle(case)
    o, LH, count, ld_f = case.opts, case.LH, case.opts["count"], hr.N_AUDIO_CTX
    got = {n: [] for n in hr.QUANTITIES["dynamic"]}
    for w in range(case.W):
        q, xkv, xkv_ptr = _device_inputs(lib, h, case, windows=[w])
        nr, F = case.rows(w), case.n_frames[w]
        lay = _layout(lib, h, 0, case.max_n, 0)
        scratch = torch.full((lay["total"],), 0xFF, dtype=torch.uint8, device="cuda")
        peaks = _peaks(case, [w], nr)
        sel_rows = _nan_filled(count, nr, ld_f)
        assert lib.swx_heads_dynamic(h, _p(q), case.max_n, case.n_sot, nr, xkv_ptr, F, o["qk_scale"], count, _p(peaks), _p(sel_rows), ld_f,
                                     _p(scratch), scratch.numel(), _stream()) == 0
        need = lib.swx_align_weights_scratch_bytes(1, count, nr)
        ascratch = torch.empty(max(need, 256), dtype=torch.uint8, device="cuda")
        out = _nan_filled(nr, ld_f)
        assert lib.swx_align_weights(_p(sel_rows), 1, count, nr, ld_f, _i32([F]), o["qk_scale"], o["width"], _p(out), _p(ascratch),
                                     ascratch.numel(), _stream()) == 0
        torch.cuda.synchronize()
        got["dscore"].append(_region(scratch, lay["score"], torch.float64, (LH, nr)))
        got["sel"].append(_region(scratch, lay["sel"], torch.int32, (nr, count)))
        got["gathered"].append(sel_rows.cpu().numpy()[:, :, :F])
        bits = out.view(torch.int32).cpu().numpy()
        assert (bits[:, F:] == np.int32(NAN_BITS)).all()
        mat = out.cpu().numpy()[:, :F].astype(np.float64)
        assert not case.matrix_compared(w) or np.isfinite(mat).all()
        got["matrix"].append(mat)
    _report(case, got, ref, "single")


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_dynamic_width_13_is_refused_and_writes_nothing(dtype):
    lib = _lib()
    case = hr.get_case(f"dyn-width11-{dtype}")
    rc, out, _, _ = _run_dynamic_batch(lib, case, width=13)
    assert rc == -3
    assert (out.view(torch.int32) == NAN_BITS).all()


# ---------------------------------------------------------------------------------------------------------------- new
def _new_args(case):
    o = case.opts
    return (o["qk_scale"], o["width"], o["topk"], o["w_col"], o["w_row"], o["w_cov"])


@pytest.mark.parametrize("name", list(NEW))
def test_new_batch_against_f64(name):
    lib = _lib()
    case = hr.get_case(name)
    ref = hr.reference(case)
    h = _handle(case)
    q, xkv, xkv_ptr = _device_inputs(lib, h, case)
    W, R, LH, topk = case.W, case.max_rows, case.LH, case.opts["topk"]
    lay = _layout(lib, h, W, case.max_n, 0)
    scratch = torch.full((lay["total"],), 0xFF, dtype=torch.uint8, device="cuda")
    out = _nan_filled(W, R, hr.N_AUDIO_CTX)
    assert lib.swx_heads_new_batch(h, _p(q), W, case.max_n, case.n_sot, _i32(case.n_tok), _i32(case.n_frames), xkv_ptr, 0, *_new_args(case),
                                   _p(out), hr.N_AUDIO_CTX, _p(scratch), scratch.numel(), _stream()) == 0
    torch.cuda.synchronize()
    colnorm = _region(scratch, lay["colnorm"], torch.float32, (W, LH, hr.HS_MAXF))
    nscore = _region(scratch, lay["nscore"], torch.float32, (W, LH))
    top = _region(scratch, lay["top"], torch.int32, (W, LH))
    got = dict(colnorm=[colnorm[w, :, :case.n_frames[w]] for w in range(W)], nscore=list(nscore), top=[top[w, :topk] for w in range(W)],
               matrix=_check_matrix_block(case, out, "batch"))
    _report(case, got, ref, "batch")


@pytest.mark.parametrize("name", [n for n in NEW if n.startswith("new-w11-cov0.5")])
def test_new_single_window_entry_against_f64(name):
    lib = _lib()
    case = hr.get_case(name)
    ref = hr.reference(case)
    h = _handle(case)
    LH, topk, ld_f = case.LH, case.opts["topk"], hr.N_AUDIO_CTX
    got = {n: [] for n in hr.QUANTITIES["new"]}
    for w in range(case.W):
        q, xkv, xkv_ptr = _device_inputs(lib, h, case, windows=[w])
        nr, F = case.rows(w), case.n_frames[w]
        lay = _layout(lib, h, 0, case.max_n, 0)
        scratch = torch.full((lay["total"],), 0xFF, dtype=torch.uint8, device="cuda")
        out = _nan_filled(nr, ld_f)
        assert lib.swx_heads_new(h, _p(q), case.max_n, case.n_tok[w], case.n_sot, nr, xkv_ptr, F, *_new_args(case), _p(out), ld_f,
                                 _p(scratch), scratch.numel(), _stream()) == 0
        torch.cuda.synchronize()
        got["colnorm"].append(_region(scratch, lay["colnorm"], torch.float32, (LH, hr.HS_MAXF))[:, :F])
        got["nscore"].append(_region(scratch, lay["nscore"], torch.float32, (LH,)))
        got["top"].append(_region(scratch, lay["top"], torch.int32, (LH,))[:topk])
        assert (out.view(torch.int32).cpu().numpy()[:, F:] == np.int32(NAN_BITS)).all()
        mat = out.cpu().numpy()[:, :F].astype(np.float64)
        assert np.isfinite(mat).all()
        got["matrix"].append(mat)
    _report(case, got, ref, "single")


# ---------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("n_in", hr.POOL_N_IN)
def test_weighted_sum_against_f64(n_in):
    lib = _lib()
    for n in hr.POOL_SIZES:
        coef, xs = hr.pool_inputs(n_in, n)
        ref, mag = hr.pool(coef, xs)
        d_xs = [torch.from_numpy(x.copy()).cuda() for x in xs]
        out = _nan_filled(n + 3)
        ptrs = (ctypes.c_void_p * n_in)(*[x.data_ptr() for x in d_xs])
        assert lib.swx_weighted_sum(ptrs, (ctypes.c_float * n_in)(*coef.tolist()), n_in, _p(out), n, _stream()) == 0
        torch.cuda.synchronize()
        r = hr.ratio(out.cpu().numpy()[:n], ref, hr.tol_pool(n_in, mag))
        print(f"headsel ratio case=pool-{n_in}x{n} call=weighted_sum pool={r:.4f}")
        assert r <= 1.0, (n_in, n, r)
        assert (out.view(torch.int32)[n:] == NAN_BITS).all()


def test_weighted_sum_refuses_nine_inputs():
    lib = _lib()
    xs = [torch.ones(256, device="cuda") for _ in range(9)]
    out = _nan_filled(256)
    ptrs = (ctypes.c_void_p * 9)(*[x.data_ptr() for x in xs])
    assert lib.swx_weighted_sum(ptrs, (ctypes.c_float * 9)(*([0.1] * 9)), 9, _p(out), 256, _stream()) == -2
    torch.cuda.synchronize()
    assert (out.view(torch.int32) == NAN_BITS).all()
