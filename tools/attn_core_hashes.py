"""One hash per attention case, for the library VP_HIP_LIB points at: the attention tap on the case of every (dtype, shape, flags) tests/test_gpu_attention.py runs, and
the fused tap on its three hot-operand cases.  Run it once per library on the same box; equal lines = equal bits.
usage: VP_HIP_LIB=<libvitpose_hip.so of a tree> python tools/attn_core_hashes.py LABEL OUTFILE   (profiles/attn_core_once_bits.txt holds both runs)"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
import attention_cases as AC  # noqa: E402
from easy_vitpose_amd import _capi as capi  # noqa: E402

label, outfile = sys.argv[1], sys.argv[2]
lib = capi.load_library()
B = 3
QSPLIT, BLOCKED, MX = 1, 2, 4
lines = []


def record(name, *arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    lines.append(f'{label}  {name}  sha256 {h.hexdigest()}')
    print(lines[-1], flush=True)


def attention(dtype, D, heads, flags):
    case = AC.case(dtype, B, D, heads)
    out = np.empty((B * AC.T, D), np.float32)
    sc = np.empty((B * AC.T, D // 32), np.uint8) if flags & MX else None
    qkv = np.ascontiguousarray(case.qkv)
    capi.check(lib.vp_dbg_attention_case(0, capi.DTYPES[dtype], B, D, heads, flags, qkv.ctypes.data, out.ctypes.data, None if sc is None else sc.ctypes.data))
    record(f'vp_dbg_attention_case {dtype} D={D} heads={heads} flags={flags}', out, *([] if sc is None else [sc]))


for dtype in ('fp16', 'bf16'):
    for D, heads in ((384, 12), (768, 12), (1280, 16)):   # head dim 32 / 64 / 80
        for flags in (0, QSPLIT):
            attention(dtype, D, heads, flags)
    for D, heads in ((768, 12), (1024, 16)):
        for flags in (BLOCKED, BLOCKED | QSPLIT):
            attention(dtype, D, heads, flags)
for flags in (MX, MX | BLOCKED):
    attention('fp16', 768, 12, flags)
for dtype, D, heads, npairs in (('fp16', 1280, 16, 8), ('bf16', 1280, 16, 9), ('fp16', 768, 12, 6)):   # gemm8.hip EPI_QKV_ATTN twice, qkvattn.hip
    x, W, bias = AC.fused_operands(dtype, D, heads, npairs)
    fused = np.empty((npairs * 384, D), np.float32)
    capi.check(lib.vp_dbg_qkvattn(0, capi.DTYPES[dtype], npairs, D, heads, x.ctypes.data, W.ctypes.data, bias.ctypes.data, fused.ctypes.data))
    record(f'vp_dbg_qkvattn {dtype} D={D} heads={heads} npairs={npairs}', fused)
os.makedirs(os.path.dirname(os.path.abspath(outfile)), exist_ok=True)
open(outfile, 'w').write('\n'.join(lines) + '\n')
