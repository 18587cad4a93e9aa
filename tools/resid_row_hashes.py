"""One hash of the outputs (residual GEMMs: planes, hi + lo as the existing taps return them, and statistics) per case, for the library VP_HIP_LIB points at:
the residual GEMMs on every tile, split-K, and the epilogues of the 8-phase kernels (16-bit and MXFP8 operands, residual, wide 16-bit and MXFP8 output).
usage: VP_HIP_LIB=<libvitpose_hip.so of the tree> python tools/resid_row_hashes.py LABEL OUTFILE   (profiles/resid_row_once_bits.txt, profiles/gemm8_epilogue_once_bits.txt)"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np
import torch

label, outfile = sys.argv[1], sys.argv[2]
lib = C.CDLL(os.environ['VP_HIP_LIB'])
lib.vp_dbg_gemm_case.argtypes = [C.c_int32] * 9 + [C.c_void_p] * 8
lib.vp_dbg_gemm_fp8_case.argtypes = [C.c_int32] * 5 + [C.c_void_p] * 8
lib.vp_last_error.argtypes = [C.c_void_p]
lib.vp_last_error.restype = C.c_char_p
DT = {'fp16': 0, 'bf16': 1}
AB, REV = 4, 8


def round_to(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.to(torch.float16 if dtype == 'fp16' else torch.bfloat16).float().numpy()


def case(epi, variant, flags, A, W, bias, aux, group_m, dtype):
    m, k = A.shape
    n = W.shape[0]
    out = np.empty((m, n), np.float32)
    stats = np.empty((m, n // 64, 2), np.float32)
    keep = [np.ascontiguousarray(a, dtype=np.float32) for a in (A, W, bias, aux)]
    rc = lib.vp_dbg_gemm_case(0, DT[dtype], epi, variant, group_m, flags, m, n, k, *[a.ctypes.data for a in keep], None, None, out.ctypes.data, stats.ctypes.data)
    assert rc == 0, lib.vp_last_error(None)
    return out, stats


lines = []


def record(name, h):
    lines.append(f'{label}  {name}  sha256 {h.hexdigest()}')
    print(lines[-1], flush=True)


D = 768
# test_residual_gemm_configurations[proj] (fp16, bf16): the module's operands fixture draws first, then the case
for dtype, M, seed in (('fp16', 192 * 64, 0), ('bf16', 192 * 40, 1)):
    rng = np.random.default_rng(seed)
    round_to(rng.standard_normal((M, D)).astype(np.float32), dtype)
    K = D
    A = round_to((rng.standard_normal((M, K)) * 1.0).astype(np.float32), dtype)
    W = round_to((rng.standard_normal((D, K)) * 0.03).astype(np.float32), dtype)
    bias = (rng.standard_normal(D) * 0.1).astype(np.float32)
    resid = (rng.standard_normal((M, D)) * 2.0).astype(np.float32)
    h = hashlib.sha256()
    for variant in (11, 8, 9, 17, 16, 18, 12, 15, 30, 31, 41, 20, 3):
        o, st = case(6, variant, 0, A, W, bias, resid, 8 if 16 <= variant <= 18 else 0, dtype)
        h.update(o.tobytes()); h.update(st.tobytes())
    record(f'test_residual_gemm_configurations[proj] {dtype}, 13 tiles', h)
# test_split_k_residual_gemm[fc2 ViTPose-B x 1]
K, Dm, rows = 3072, 768, 192
rng = np.random.default_rng(K + rows)
A = round_to((rng.standard_normal((rows, K)) * 0.5).astype(np.float32), 'fp16')
W = round_to((rng.standard_normal((Dm, K)) * 0.03).astype(np.float32), 'fp16')
bias = (rng.standard_normal(Dm) * 0.1).astype(np.float32)
resid = (rng.standard_normal((rows, Dm)) * 2.0).astype(np.float32)
h = hashlib.sha256()
o, st = case(6, 12, AB, A, W, bias, resid, 0, 'fp16')
h.update(o.tobytes()); h.update(st.tobytes())
for S in (2, 4, 8):
    for variant in (12, 1, 11, 15, 20, 30, 31):
        o, st = case(6, variant, AB | (S << 8), A, W, bias, resid, 0, 'fp16')
        h.update(o.tobytes()); h.update(st.tobytes())
record('test_split_k_residual_gemm[fc2 ViTPose-B x 1], unsplit + S 2/4/8 x 7 tiles', h)


def fp8_operands(M, N, K, seed):   # tests/test_gpu_fp8.py::_operands
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((M, K)).astype(np.float32)
    A *= np.repeat(np.exp2(rng.integers(-3, 4, size=(M, K // 32))).astype(np.float32), 32, axis=1)
    A[:, 3] += (np.arange(M) % 7).astype(np.float32)
    A[5, 40] = 300.0
    W = (rng.standard_normal((N, K)) * 0.04).astype(np.float32)
    W[:, 1] += 0.1 * (np.arange(N) % 5)
    bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
    return rng, A, W, bias


def fp8_case(epi, A, W, bias, aux=None):
    (M, K), N = A.shape, W.shape[0]
    out = np.empty((M, N), np.float32)
    stats = np.empty((M, N // 64, 2), np.float32) if epi == 6 else None
    a_deq, w_deq = np.empty((M, K), np.float32), np.empty((N, K), np.float32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (A, W, bias, aux)]
    rc = lib.vp_dbg_gemm_fp8_case(0, epi, M, N, K, *[None if a is None else a.ctypes.data for a in keep], out.ctypes.data,
                                  None if stats is None else stats.ctypes.data, a_deq.ctypes.data, w_deq.ctypes.data)
    assert rc == 0, lib.vp_last_error(None)
    h = hashlib.sha256()
    h.update(out.tobytes())
    if stats is not None:
        h.update(stats.tobytes())
    return h


# test_fp8_gemm_residual_epilogue: 512-768-768 = 256 x 192 tiles through LDS, 512-1024-4096 = 256 x 256 tiles straight from registers
for M, N, K in ((512, 768, 768), (512, 1024, 4096)):
    rng, A, W, bias = fp8_operands(M, N, K, M + 2 * N)
    A *= 0.5
    resid = (rng.standard_normal((M, N)) * 2.0).astype(np.float32)
    record(f'test_fp8_gemm_residual_epilogue[{M}-{N}-{K}]', fp8_case(6, A, W, bias, resid))
# test_fp8_gemm_qkv_epilogue[512-2304-768] (16-bit output), test_fp8_gemm_fc1_epilogue_writes_mxfp8[512-3072-768] (MXFP8 output)
_, A, W, bias = fp8_operands(512, 2304, 768, 512 + 2304)
record('test_fp8_gemm_qkv_epilogue[512-2304-768]', fp8_case(0, A, W, bias))
_, A, W, bias = fp8_operands(512, 3072, 768, 512 * 3 + 3072)
record('test_fp8_gemm_fc1_epilogue_writes_mxfp8[512-3072-768]', fp8_case(1, A, W, bias))


# the wide 16-bit epilogues of the 8-phase kernel (tests/test_gpu_gemm_cfgs.py::_wide_gemm_configurations): qkv and fc1 (GELU, 64 x 64-blocked output), with the
# LayerNorm-consumer fold and without, 256 x 256 and 192 x 256 tiles at 40 crops (workgroups with one and with two tiles), 192 x 256 at 25 crops
def wide_case(epi, variant, flags, A, W, bias, rowstat, ln_s, dtype):
    m, n = A.shape[0], W.shape[0]
    out = np.empty((m, n), np.float32)
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float32) for a in (A, W, bias, None, rowstat, ln_s)]
    rc = lib.vp_dbg_gemm_case(0, DT[dtype], epi, variant, 8, flags, m, n, A.shape[1], *[None if a is None else a.ctypes.data for a in keep], out.ctypes.data, None)
    assert rc == 0, lib.vp_last_error(None)
    return out


OUTB = 2
for dtype, seed in (('fp16', 0), ('bf16', 1)):
    rng = np.random.default_rng(seed)
    M = 192 * 40
    A = round_to(rng.standard_normal((M, D)).astype(np.float32), dtype)
    for name, N, epi, flags in (('qkv', 3 * D, 0, 0), ('fc1', 4 * D, 1, OUTB)):
        W = round_to((rng.standard_normal((N, D)) * 0.05).astype(np.float32), dtype)
        bias = (rng.standard_normal(N) * 0.1).astype(np.float32)
        rowstat = np.stack([rng.standard_normal(M) * 0.2, 1.0 + 0.3 * rng.random(M)], 1).astype(np.float32)
        ln_s = W.astype(np.float64).sum(1).astype(np.float32)
        h = hashlib.sha256()
        for variant, rows in ((16, M), (18, M), (18, 192 * 25)):
            h.update(wide_case(epi, variant, flags, A[:rows], W, bias, rowstat[:rows], ln_s, dtype).tobytes())   # fold
            h.update(wide_case(epi, variant, flags, A[:rows], W, bias, None, None, dtype).tobytes())             # plain bias
        record(f'wide 16-bit epilogue {name} {dtype}{", blocked output" if flags & OUTB else ""}: fold + no fold x (variant 16, 18 at 40 crops; 18 at 25 crops)', h)
os.makedirs(os.path.dirname(outfile), exist_ok=True)
open(outfile, 'w').write('\n'.join(lines) + '\n')
