"""CPU-side code-object screen of the LDS-DMA ViT attention kernel (csrc/attn16_dma.hip), in the style of test_isa_screen.py: hipcc
cross-compiles gfx950, no GPU needed.  The kernel is designed for three workgroups of four waves per CU (one head per workgroup, K and V
single-buffered: 53,248 B of LDS each), i.e. three waves per SIMD: at most 168 VGPRs, no scratch, no spilled VGPR — a scratch reload is
followed by `s_waitcnt vmcnt(0)`, which would drain the LDS-DMA pieces and the Q loads in flight in the middle of a block."""
import os
import re

from test_isa_screen import CSRC, _kernel_meta, _opsel_sites

SRC = os.path.join(CSRC, "attn16_dma.hip")


def test_dma_attention_instantiations_have_no_scratch_and_keep_two_waves_per_simd(tmp_path):
    meta, txt = _kernel_meta(SRC, tmp_path)
    kernels = {k: v for k, v in meta.items() if "attention16_dma_kernel" in k}
    assert len(kernels) == 2                          # fp16 and bf16
    for name, m in kernels.items():
        assert m["scratch"] == 0 and m["vgpr_spill"] == 0, (name, m)
        assert m["vgpr"] <= 168, (name, m)            # three waves per SIMD (one head per workgroup: three workgroups of 53,248 B per CU)
    # the ablation knob of the tool builds must not be in the product build
    assert "ATTN_DEBUG_BITS" not in open(os.path.join(CSRC, "Makefile")).read()


def test_dma_attention_has_no_packed_fp32_op_sel_broadcast_straight_behind_an_lds_wait():
    sites = _opsel_sites(_kernel_meta(SRC)[1])
    assert not sites, f"attn16_dma.hip: hi->lo op_sel packed fp32 operations straight behind an lgkmcnt wait at assembly lines {sites[:8]}"


def test_dma_attention_waits_for_vector_memory_only_where_the_source_says_so():
    """Every `s_waitcnt vmcnt` of the kernel is one of the counted waits of the source: hipcc's own wait insertion must not add one (it
    does for a plain global load, and for a transposed LDS read behind an LDS-DMA it knows about: both are issued from inline asm)."""
    _, txt = _kernel_meta(SRC)
    lines = txt.split("\n")
    assert sum("vmcnt" in l for l in lines) >= 8            # four counted waits per instantiation at least
    for i, l in enumerate(lines):
        if "s_waitcnt" in l and "vmcnt" in l:
            assert "sched_barrier" in lines[i - 1] and "sched_barrier" in lines[i + 1], (i, l)


def test_the_fixed_q_registers_belong_to_the_inline_asm_alone():
    """The Q loads land in v[160:167], named in the asm text; between a request and the copy behind its wait nothing else may live there.  The
    register allocator is not told: the kernel needs fewer registers, and this fails when a compiler-generated instruction reaches v160."""
    _, txt = _kernel_meta(SRC)
    in_asm, top = False, 0
    for l in txt.split("\n"):
        t = l.strip()
        if "#ASMSTART" in t or "#ASMEND" in t:
            in_asm = "#ASMSTART" in t
            continue
        if in_asm or not t or t[0] in ";.":
            continue
        for m in re.finditer(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]", t):
            top = max(top, int(m.group(1) or m.group(3)))
    assert 100 < top < 160, top
