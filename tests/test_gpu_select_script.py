"""The selection path of the decoding loop (csrc/swx_decode.hip: logit filters, decode_select_kernel, decode_select_reg_kernel<51>,
decode_beam_update_kernel, decode_step_finish_kernel, decode_finalize_kernel) on scripted logits, through swx_test_decode_script,
against the oracle's own filter and decoder classes (tests/select_script.py).  Every case runs on the register kernel and on the
memory-walking kernel (debug flag 8192); both must equal the reference, not merely each other.

Exact: tokens, lens (-1 slots included), steps executed, ancestor table, pos0.  sum_logprobs: atol 1e-4 (at most 24 steps of a few
f32 ulp at magnitude <= 30; scripted finite logits lie in [-20, 20]); no_speech_prob: 1e-4 + 1e-2 * ref.  The decision margins of
every case are >= 1e-3 in float64 (tests/test_select_script_cpu.py), so no f32 rounding can move a decision.

The hashed_* and top_bucket_* cases run the kernels' BUILT-IN sampling draw (noise = NULL) against the float64 statement of it in
tests/sampler_ref.py; there the margin also covers the f32 error of the variate itself, at most 4.9e-4 outside the outermost
2^-12 of the buckets (tests/test_gpu_sampler.py).
"""
import ctypes

import numpy as np
import pytest
import torch

import select_script as ss

pytestmark = pytest.mark.gpu

SELECT_MEM = 8192


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def run_gpu(case, mem_kernel):
    from stable_ts_amd import _lib
    lib = _lib.load()
    tok, W, G, V, n_ctx = case.tok, case.W, case.G, case.V, case.n_ctx
    M, TS, Go = W * G, n_ctx + 1, ss.g_out(case)
    dev = "cuda:0"
    begins = case.begins
    n_init = max(begins)
    init = np.full((W, n_init), tok.eot, np.int32)
    for w, t in enumerate(case.init):
        init[w, :len(t)] = t
    hb = (ctypes.c_int32 * W)(*begins)
    noise = None if case.noise is None else torch.from_numpy(case.noise).to(dev)
    # (a hashed case: noise stays NULL and the kernels draw from cfg.seed / cfg.window_uid)
    uid = None if case.window_uid is None else (ctypes.c_int32 * W)(*case.window_uid)
    cfg = _lib.swx_decode_cfg(
        n_windows=W, n_group=G, beam=case.beam, temperature=case.temperature, patience=case.patience,
        sample_len=case.sample_len, sample_begin=n_init, sot_index=0, suppress_blank=case.suppress_blank,
        apply_timestamp_rules=case.rules, max_initial_timestamp_index=case.max_initial, eot=tok.eot, sot=tok.sot,
        no_timestamps=tok.no_timestamps, timestamp_begin=tok.timestamp_begin, no_speech=tok.no_speech, blank_token=tok.blank,
        n_suppress=len(case.suppress), min_tokens=case.min_tokens, seed=case.seed,
        window_uid=None if uid is None else ctypes.cast(uid, ctypes.POINTER(ctypes.c_int32)),
        noise=noise.data_ptr() if noise is not None else None,
        sample_begins=ctypes.cast(hb, ctypes.POINTER(ctypes.c_int32)) if min(begins) != n_init else None, sot_indices=None)
    d_init = torch.from_numpy(init).to(dev)
    d_sup = torch.tensor(case.suppress, dtype=torch.int32, device=dev) if case.suppress else None
    d_mask = torch.from_numpy(case.ts_mask).to(dev) if case.ts_mask is not None else None
    d_pre = torch.from_numpy(case.prefill).to(dev)
    d_scr = torch.from_numpy(case.script).to(dev) if case.script.shape[0] else None
    tokens = torch.full((W, Go, TS), -7, dtype=torch.int32, device=dev)
    lens = torch.full((W, Go), -7, dtype=torch.int32, device=dev)
    sumlp = torch.full((W, Go), float("nan"), device=dev)
    nosp = torch.zeros(W, device=dev)
    anc = torch.full((M, n_ctx), -7, dtype=torch.int32, device=dev)
    pos0 = torch.full((M,), -7, dtype=torch.int32, device=dev)
    nbytes = lib.swx_test_decode_script_ws_bytes(ctypes.byref(cfg), V, n_ctx)
    assert nbytes > 0
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    off = (-ws.data_ptr()) % 256
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    old = lib.swx_debug_flags(-1)
    lib.swx_debug_flags((old | SELECT_MEM) if mem_kernel else (old & ~SELECT_MEM))
    try:
        torch.cuda.synchronize()
        steps = lib.swx_test_decode_script(ctypes.byref(cfg), V, n_ctx, _p(d_init), _p(d_sup), _p(d_mask), _p(d_pre), _p(d_scr),
                                           case.script.shape[0], _p(tokens), _p(lens), _p(sumlp), _p(nosp), _p(anc), _p(pos0),
                                           ctypes.c_void_p(ws.data_ptr() + off), nbytes, stream)
    finally:
        lib.swx_debug_flags(old)
    _lib.check(steps, "swx_test_decode_script")
    return dict(steps=steps, tokens=tokens.cpu().numpy(), lens=lens.cpu().numpy(), sumlp=sumlp.cpu().numpy().astype(np.float64),
                nospeech=nosp.cpu().numpy().astype(np.float64), anc=anc.cpu().numpy(), pos0=pos0.cpu().numpy())


_MAKERS = list(ss.all_cases())
_REFS = {}


def _case_and_ref(k):
    """the reference of a case is computed once and shared by its two kernel runs; the logits are rebuilt, not kept"""
    case = _MAKERS[k]()
    if k not in _REFS:
        _REFS[k] = ss.run_reference(case)
    return case, _REFS[k]


@pytest.mark.parametrize("mem_kernel", [0, 1], ids=["reg", "mem"])
@pytest.mark.parametrize("k", range(len(_MAKERS)))
def test_scripted_selection_equals_reference(k, mem_kernel):
    case, ref = _case_and_ref(k)
    got = run_gpu(case, mem_kernel)
    name = case.name
    used = ref.lens >= 0
    assert got["lens"].tolist() == ref.lens.tolist(), name
    assert got["tokens"][used].tolist() == ref.tokens[used].tolist(), name
    assert got["steps"] == ref.steps, name
    assert got["pos0"].tolist() == ref.pos0.tolist(), name
    if ref.anc is not None:
        assert got["anc"].tolist() == ref.anc.tolist(), name
    err = np.abs(got["sumlp"][used] - ref.sumlp[used])
    print(name, "max |sum_logprobs - ref| =", np.nanmax(err) if err.size else 0.0)
    # (equal_nan / equal infinities: where the reference's own sum is not finite the kernel's must be the same non-finite value)
    same = (got["sumlp"][used] == ref.sumlp[used]) | (np.isnan(got["sumlp"][used]) & np.isnan(ref.sumlp[used]))
    assert (same | (err <= 1e-4)).all(), (name, got["sumlp"], ref.sumlp)
    assert (np.abs(got["nospeech"] - ref.nospeech) <= 1e-4 + 1e-2 * ref.nospeech).all(), name
