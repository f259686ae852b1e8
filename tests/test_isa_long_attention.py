"""CPU-side screen of the streaming-softmax attention kernel (no GPU needed: hipcc cross-compiles gfx950): csrc/attn16_long.hip compiled to
assembly as tests/test_isa_screen.py does, and the code-object metadata of every kernel in it read — no scratch, no spilled VGPR.  A wave
carries the running maximum, sum and context of four query blocks across the chunk loop next to the prefetched K / V rows of the next
chunk; a spill there would put scratch traffic (and an `s_waitcnt vmcnt(0)` per reload) into every chunk of every query block."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "iisan_amd", "csrc", "attn16_long.hip")


def _asm(src):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    out = os.path.join(tempfile.mkdtemp(prefix="iisan_isa_"), os.path.basename(src) + ".s")
    try:
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", src, "-o", out],
                              stderr=subprocess.DEVNULL)
        with open(out) as f:
            return f.read()
    finally:
        shutil.rmtree(os.path.dirname(out), ignore_errors=True)


def test_long_attention_kernels_have_no_scratch_and_no_spilled_vgpr():
    assert os.path.exists(SRC), "csrc/attn16_long.hip is missing"
    txt = _asm(SRC)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", txt, re.S):
        get = lambda k: int(re.search(k + r":\s*(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = dict(vgpr=get(r"\.vgpr_count"), vgpr_spill=get(r"\.vgpr_spill_count"), scratch=get(r"\.private_segment_fixed_size"),
                                lds=int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", txt[:m.start()].rsplit("- .agpr_count", 1)[-1]).group(1)))
    kernels = {k: v for k, v in meta.items() if "attention16_long_kernel" in k}
    assert len(meta) == len(kernels) == 2, sorted(meta)              # F16 and BF16, and nothing else in the file
    for name, v in kernels.items():
        print(name, v)
        assert v["scratch"] == 0, (name, v)
        assert v["vgpr_spill"] == 0, (name, v)
        assert v["vgpr"] <= 256, (name, v)                           # two waves per SIMD: the two workgroups per CU the launch bounds ask for
        assert v["lds"] <= 64 * 1024, (name, v)                      # static LDS: K + V^T + key limits of one 128-key chunk
