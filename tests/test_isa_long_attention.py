"""CPU-side screen of the streaming-softmax attention kernels (no GPU needed: hipcc cross-compiles gfx950): csrc/attn16_long.hip and
csrc/attn16_hd80.hip — the two geometries of the chunk walk in csrc/attn16_stream.h — compiled to assembly as tests/test_isa_screen.py
does, and the code-object metadata of every kernel in them read — no scratch, no spilled VGPR.  A wave carries the running maximum, sum
and context of four (80-wide heads: three) query blocks across the chunk loop next to the prefetched K / V rows of the next chunk; a spill
there would put scratch traffic (and an `s_waitcnt vmcnt(0)` per reload) into every chunk of every query block.  The 80-wide kernel sits
at 255 of the 256 registers that two waves per SIMD allow."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "iisan_amd", "csrc")


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


@pytest.mark.parametrize("fname,kernel", [("attn16_long.hip", "attention16_long_kernel"), ("attn16_hd80.hip", "attention16_hd80_kernel")])
def test_long_attention_kernels_have_no_scratch_and_no_spilled_vgpr(fname, kernel):
    src = os.path.join(CSRC, fname)
    assert os.path.exists(src), f"csrc/{fname} is missing"
    txt = _asm(src)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n(.*?)\.wavefront_size", txt, re.S):
        get = lambda k: int(re.search(k + r":\s*(\d+)", m.group(2)).group(1))
        meta[m.group(1)] = dict(vgpr=get(r"\.vgpr_count"), vgpr_spill=get(r"\.vgpr_spill_count"), scratch=get(r"\.private_segment_fixed_size"),
                                lds=int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", txt[:m.start()].rsplit("- .agpr_count", 1)[-1]).group(1)))
    kernels = {k: v for k, v in meta.items() if kernel in k}
    assert len(meta) == len(kernels) == 2, sorted(meta)              # F16 and BF16, and nothing else in the file
    assert sum("I3F16E" in k for k in kernels) == 1 and sum("I4BF16E" in k for k in kernels) == 1, sorted(kernels)
    for name, v in kernels.items():
        print(name, v)
        assert v["scratch"] == 0, (name, v)
        assert v["vgpr_spill"] == 0, (name, v)
        assert v["vgpr"] <= 256, (name, v)                           # two waves per SIMD: the two workgroups per CU the launch bounds ask for
        assert v["lds"] <= 64 * 1024, (name, v)                      # static LDS: K + V^T + key limits of one 128-key chunk
    if fname == "attn16_hd80.hip":
        # the score chain stays three 32-slot steps: a chain ending in a 16x16x16 step gave schedule-dependent scores (profiles/vit_huge.md §4)
        assert "v_mfma_f32_16x16x16" not in txt
