"""Compile-time properties the performance claims rest on (README / DESIGN): the fused inference kernels hold everything in
registers -- no VGPR spills, no scratch -- and the weight streams use the buffer form of the LDS-DMA.  Checked by compiling
the two translation units for gfx950 with hipcc's resource-usage remarks (no GPU needed; ~1 min, both units in parallel)."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "moco_flow_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--cuda-device-only",
         "-Rpass-analysis=kernel-resource-usage", "-S", "-o"]


def _unit_flags(unit):
    """the unit's own flags of the shipped build (csrc/Makefile, `unitflags`)"""
    return subprocess.run(["make", "-s", "unitflags", f"UNIT={unit}"], cwd=CSRC, capture_output=True, text=True, check=True).stdout.split()


def _compile(unit, extra):
    out = f"/tmp/mf_props_{os.getpid()}_{unit}.s"
    r = subprocess.run([HIPCC] + FLAGS + [out] + extra + [unit + ".hip"], cwd=CSRC, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(out).read()
    os.remove(out)
    usage = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[(?:bytes/lane|waves/SIMD)\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    return usage, asm


def _scratch_distance_to_mfma(asm, mangled):
    """Smallest distance, in INSTRUCTIONS, between a scratch access and a matrix instruction inside kernel `mangled` (a large
    number when the kernel has no scratch access)."""
    body, on = [], False
    for line in asm.splitlines():
        if line.startswith(mangled + ":"):
            on = True
        if on:
            t = line.strip()
            if t and not t.startswith((";", ".", "//")) and not t.endswith(":"):
                body.append(t)
            if "s_endpgm" in line:
                break
    sc = [i for i, t in enumerate(body) if t.startswith("scratch_")]
    mf = [i for i, t in enumerate(body) if t.startswith("v_mfma")]
    return min((abs(i - j) for i in sc for j in mf), default=10 ** 9)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_shipped_inference_kernels_have_no_spills_and_stream_weights_by_buffer_dma():
    with ThreadPoolExecutor(4) as ex:
        f32 = ex.submit(_compile, "mf_render", [])
        b16 = ex.submit(_compile, "mf_render_bf16", _unit_flags("mf_render_bf16"))      # csrc/Makefile builds this unit so
        bw3 = ex.submit(_compile, "mf_backward_bf16", _unit_flags("mf_backward_bf16"))
        nb3 = ex.submit(_compile, "mf_nofgrad_bf16", _unit_flags("mf_nofgrad_bf16"))
        assert "-fno-slp-vectorize" in _unit_flags("mf_render_bf16") and not _unit_flags("mf_render")
        (u32, a32), (u16, a16), (ub3, _) = f32.result(), b16.result(), bw3.result()
    u16 = {**u16, **{k: v for k, v in ub3.items() if "nerf_backward_kernel_x3" in k}}
    # the NoF backward in three products: no spills, no scratch, and small enough for TWO workgroups per CU (its host code
    # launches two per CU: 256 registers and a third of the LDS each)
    nofs = [v for k, v in nb3.result()[0].items() if "nof_backward_kernel_x3" in k]
    assert len(nofs) == 2                                         # <BITS = false | true>
    for unb in nofs:
        assert unb["VGPRs Spill"] == 0 and unb["ScratchSize"] == 0 and unb["VGPRs"] + unb["AGPRs"] <= 256 and unb["Occupancy"] == 2, unb
    # render_kernel<MOCO, DUMP>: the two inference instantiations (DUMP = false) and every bf16 kernel
    x3 = [k for k in u16 if re.search(r"render_kernel_bf16ILb[01]ELb1ELb[01]E", k) or      # <MOCO, X3 = true, DUMP>
          re.search(r"points_kernel_bf16ILb[01]ELb0ELb1E", k) or                           # <NOF, PERPT = false, X3 = true>
          "nerf_backward_kernel_x3" in k]                                                 # the three-product dX chain
    want = [k for k in u32 if re.search(r"render_kernelILb[01]ELb0EE", k)] + \
           [k for k in u16 if ("render_kernel_bf16" in k or "points_kernel_bf16" in k) and k not in x3]
    assert len(want) == 2 + 5 and len(x3) == 8, sorted(list(u32) + list(u16))   # fp32 NeRF / MoCo; bf16 render x 2, point query x 3; x3: NeRF, MoCo, NeRF + dump, MoCo + dump (round 5), point query x 2, dX chain x 2
    for k in want:
        u = {**u32, **u16}[k]
        assert u["VGPRs"] <= 256, (k, u)
        # round 6: the fast bf16 kernels are back at zero too.  Round 5's pipelined tile (two accumulator sets in flight) had pushed
        # 17 / 11 dwords into scratch -- not per-tile bookkeeping of the tile loop but loop-INVARIANT per-lane values hipcc had
        # hoisted out of the whole group loop: the embedding evaluations' half-dependent component indices and table addresses,
        # a VGPR copy of G for a 64-bit compare, the lane's sample slot (csrc/mf_bf16.hpp opaque_lane_half, mf_render_bf16.hip
        # group_rays / the per-tile v_mbcnt).  Re-derived where they are used they cost a v_cndmask each in a VALU phase.
        assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
    # the bf16x3 kernels hold (hi, lo) pairs of a 256-wide layer's input AND output: one wave per SIMD with the whole register
    # file -- 256 VGPRs + AGPRs (hipcc parks finished output tiles there), nothing in scratch
    for k in x3:
        assert u16[k]["VGPRs Spill"] == 0 and u16[k]["ScratchSize"] == 0, (k, u16[k])
        assert u16[k]["VGPRs"] <= 256 and u16[k]["AGPRs"] <= 256 and u16[k]["Occupancy"] == 1, (k, u16[k])
    for asm in (a32, a16):
        assert "global_load_lds" not in asm                       # FLAT-encoded LDS-DMA: forces lgkmcnt(0) waits
        assert len(re.findall(r"buffer_load_dwordx4 .* lds", asm)) > 50
    # the bf16 unit must hold no packed-fp32 VALU op (run-to-run differences on MI355X, csrc/Makefile)
    assert not re.search(r"v_pk_(mul|fma|add)_f32", a16)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_training_kernels_have_no_scratch():
    """Every 512-thread, two-waves-per-SIMD kernel of the training path (the dumping forwards, the two backward chains,
    the weight-gradient launch, the NoF evaluation / backward nodes) compiles without VGPR spills and without scratch.
    Round 2's build had 114 spilled VGPRs + 460 B/lane in wgrad_kernel (hipcc hoisted the lane-derived offsets of all
    eight block shapes in front of the item loop) and 12 / 3 in the two dumping forwards (per-sample bookkeeping carried
    across the MFMA section).  The one exception is documented: the MoCo training forward keeps <= 4 spilled dwords, all
    written in the kernel prologue and re-read at most twice per 128-sample tile (outside every MFMA loop)."""
    units = ["mf_wgrad", "mf_forward", "mf_backward", "mf_nofgrad", "mf_render"]
    with ThreadPoolExecutor(3) as ex:
        results = list(ex.map(lambda u: _compile(u, []), units))
    usage = {}
    for u, _ in results:
        usage.update(u)
    # (nof_forward_kernel<16>: the module-level forward of the reference's bare NoF() -- W = 256, round 5 -- is an envelope case, not a
    #  performance path: 64 activation registers more than the 128-wide instantiation, 46 of them spilled)
    big = {k: v for k, v in usage.items() if v.get("VGPRs", 0) >= 128 and "nof_forward_kernelILi16" not in k}   # the MFMA kernels (all launch_bounds(512, 2))
    names = " ".join(big)
    for frag in ("wgrad_kernel", "nerf_forward_kernelILb1", "nerf_backward_kernel", "nof_backward_kernel", "nof_points_dump_kernel",
                 "render_kernelILb1ELb1", "render_kernelILb0ELb1", "nof_forward_kernel"):
        assert frag in names, (frag, sorted(big))
    for k, u in big.items():
        assert u["VGPRs"] <= 256, (k, u)
        if "render_kernelILb1ELb1" in k:                   # <MOCO, DUMP>: the MoCo training forward
            assert u["VGPRs Spill"] <= 4 and u["ScratchSize"] <= 96, (k, u)    # (round 4: + the mask-row pointer; 20 B of scratch)
        else:
            assert u["VGPRs Spill"] == 0 and u["ScratchSize"] == 0, (k, u)
