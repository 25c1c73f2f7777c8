"""Hardware check of the FIRST launches of a process on the three GEMM kernels that ask for more than 64 KB of dynamic LDS:
gemm_f16_ring<64, 3> (72 KB, force_kernel 10), gemm_f16_ring<128, 3> (96 KB, 11) (csrc/swx_gemm_tiled.hip) and gemm_f16_big8 (128 KB, 12)
(csrc/swx_gemm_big.hip).  Each takes its grant (csrc/swx_common.h::swx_launch_lds) on its first launch on a device, so the very first
GEMM launches of this process are those three, in that order; every call must return 0, and every result must equal the
register-staged gemm_f16_tiled (1) on the same operands BIT FOR BIT (the same MFMA sequence per accumulator).  Shapes: the smallest
at which these kernels can still go wrong -- partial row and column tiles throughout; ring: K = 128 (two K steps for three
stages) and K = 320 (an odd step count); 256 x 256: K = 128 (the prologue holds the whole K) and K = 192 (an odd tile count).
Bias + f16 residual, ldc = ldr = N.  Exit code 0 = all agree.

    python tests/hw_checks/gemm_first_launch_check.py
"""
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

EPI_BIAS, EPI_RES = 1, 4


def main() -> int:
    from stable_ts_amd import _lib
    lib = _lib.load()
    _lib.require_gpu()
    dev = "cuda:0"
    g = torch.Generator(device="cpu").manual_seed(11)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    # (force_kernel, M, N, K) in launch order: the first three are the first launch of each kernel
    cases = [(10, 260, 136, 128), (11, 260, 136, 128), (12, 260, 264, 128), (10, 260, 136, 320), (11, 260, 136, 320), (12, 260, 264, 192)]
    ops = {}
    for (_, M, N, K) in cases:
        if (M, N, K) not in ops:
            ops[(M, N, K)] = ((torch.randn(M, K, generator=g) * 0.5).half().to(dev), (torch.randn(N, K, generator=g) * 0.03).half().to(dev),
                              torch.randn(N, generator=g).float().to(dev), torch.randn(M, N, generator=g).half().to(dev))

    def run(force, M, N, K):
        a, w, bias, res = ops[(M, N, K)]
        c = torch.full((M, N), float("nan"), dtype=torch.half, device=dev)
        rc = lib.swx_test_gemm(1, p(a), K, p(w), p(bias), p(res), p(c), N, M, N, K, EPI_BIAS | EPI_RES, force, st)
        torch.cuda.synchronize()
        return rc, c

    outs = [run(*case) for case in cases]                 # the kernels under test first ...
    bad = 0
    for (force, M, N, K), (rc, c) in zip(cases, outs):
        rc1, c1 = run(1, M, N, K)                          # ... the reference after them
        ok = rc == 0 and rc1 == 0 and not bool(torch.isnan(c).any()) and torch.equal(c, c1)
        print(("ok   " if ok else "FAIL ") + f"force {force} M={M} N={N} K={K}: rc = {rc} (tiled {rc1}); "
              f"differing elements: {int((c != c1).sum()) if rc == 0 and rc1 == 0 else -1}")
        bad += not ok
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
