#!/usr/bin/env python3
"""Static checks on the gfx950 ISA of the field kernels, run by `__graft_entry__.build()` and by
tests/test_abi_cpu.py on the very objects that are linked into libmnrf_hip.so (the device code object
is unbundled from csrc/*.o and disassembled: ~1 s per object, no recompilation).

The A-operand reads of the field kernels are hand-placed `ds_read_b128` with counted
`s_waitcnt lgkmcnt(n)`; the weight stream of the split kernels lands behind counted `s_waitcnt
vmcnt(n)`.  A counted lgkmcnt wait is only valid while nothing that returns out of order shares the
counter: scalar-memory loads do.  Asserted, per kernel that carries the hand-placed scheme (forward,
activation-gradient and second-order kernels of both arithmetics):
  * no s_load / s_buffer_load between the first and the last MFMA,
  * the hand-placed reads and counted waits are present,
  * no scratch (spill) traffic at all in the forward kernels of the split arithmetic and inside the MFMA range of
    the fp32 forward kernels; the known phase-boundary spills of the gradient kernels are reported, and bounded,
  * the weight-gradient GEMMs (mnrf_dw.o, mnrf_dwp.o) do not spill,
  * the forward-only split kernels (h2, h3) convert a value pair in the short form (mnrf_field_split_common.inc split2): the body
    of a 256-wide trunk layer loop (the `#pragma unroll 1` loops of L2-L4 and L6-L8: 384 MFMAs per 16 samples of a wave) holds no
    more non-MFMA vector instructions than the short form's count plus an allowance -- a compiler or source change that brings the
    11-instruction form back adds 3 per pair, 288 per loop at 48 samples per wave -- and nothing within two instructions of a
    v_fma_mixhi_f16 names its destination (the wait states inline assembly owes, see split2).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mirror_nerf_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"


def disassemble(obj):
    """ISA text of the gfx950 code object embedded in a hipcc-built .o -> {kernel symbol: [instruction lines]}."""
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj, os.path.join(d, "copy.o")], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}", "--unbundle"], check=True)
        text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    kernels, cur = {}, None
    for line in text.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\w+)>:", line)
        if m:
            cur = kernels.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(line)
    return kernels


def _address(line):
    m = re.search(r"// ([0-9A-Fa-f]{8,}):", line)
    return int(m.group(1), 16) if m else None


def layer_loops(body, n_mfma):
    """Non-MFMA vector instruction counts of the loops (a backward conditional branch and its target) that hold n_mfma MFMAs."""
    addr = [_address(l) for l in body]
    out = []
    for i, l in enumerate(body):
        m = re.match(r"\ts_cbranch_\w+ .*<[^>]*\+0x([0-9a-f]+)>", l)
        if m and addr[i] is not None and addr[0] is not None:
            target = addr[0] + int(m.group(1), 16)
            if target < addr[i] and target in addr:
                seg = body[addr.index(target):i + 1]
                if sum("v_mfma" in x for x in seg) == n_mfma:
                    out.append(sum(bool(re.match(r"\tv_(?!mfma)", x)) for x in seg))
    return out


def mixhi_near_readers(body):
    """Instructions within two of a v_fma_mixhi_f16 that name its destination register."""
    bad = []
    for i, l in enumerate(body):
        m = re.match(r"\tv_fma_mixhi_f16 v(\d+),", l)
        if not m:
            continue
        r = int(m.group(1))
        for nxt in body[i + 1:i + 3]:
            ins = nxt.split("//")[0]
            regs = {int(a) for a in re.findall(r"\bv(\d+)\b", ins)}
            for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", ins):
                regs |= set(range(int(a), int(b) + 1))
            if r in regs:
                bad.append(ins.strip())
    return bad


def check_object(name, mfma, rules):
    """rules: list of (regex on the kernel symbol, dict(min_counted, counted_re, scratch_inside_max, scratch_total_max))."""
    path = os.path.join(CSRC, name)
    if not os.path.exists(path):
        print(f"{path} missing: build first (make -C mirror_nerf_amd/csrc)")
        return False, 0
    ok, n = True, 0
    for sym, body in disassemble(path).items():
        rule = next((r for pat, r in rules if re.search(pat, sym)), None)
        if rule is None:
            continue
        n += 1
        mf = [i for i, l in enumerate(body) if mfma in l]
        if not mf:
            print(f"{sym}: no {mfma} found")
            ok = False
            continue
        inner = body[mf[0]:mf[-1] + 1]
        smem = [l for l in inner if re.search(r"\bs_(buffer_)?load_", l)]
        scratch_in = sum("scratch_" in l for l in inner)
        scratch_all = sum("scratch_" in l for l in body)
        reads = sum("ds_read_b128" in l for l in inner)
        counted = sum(bool(re.search(rule["counted_re"], l)) for l in inner)
        dma = sum("global_load_lds_dwordx4" in l for l in body)
        print(f"{sym}: {len(mf)} MFMA, {reads} ds_read_b128, {dma} LDS-DMA pieces, {counted} counted waits, "
              f"{len(smem)} scalar loads inside, scratch ops {scratch_in} inside / {scratch_all} total")
        if smem or counted < rule["min_counted"] or scratch_in > rule["scratch_inside_max"] \
                or scratch_all > rule["scratch_total_max"]:
            print("   ^^^ VIOLATION")
            ok = False
        if "layer_valu_max" in rule:
            loops = layer_loops(body, rule["layer_mfma"])
            near = mixhi_near_readers(body)
            print(f"   256-wide layer loops: {loops} non-MFMA vector instructions (bound {rule['layer_valu_max']}), "
                  f"{sum('v_fma_mixhi_f16' in l for l in body)} v_fma_mixhi_f16, {len(near)} with a reader within two instructions")
            if len(loops) != 2 or max(loops) > rule["layer_valu_max"] or near:
                print("   ^^^ VIOLATION (conversion form)", near[:4])
                ok = False
    return ok, n


def main():
    ok = True
    fwd32 = dict(min_counted=100, counted_re=r"s_waitcnt lgkmcnt\([1-4]\)", scratch_inside_max=0, scratch_total_max=10**6)
    grad32 = dict(fwd32, scratch_inside_max=200)
    o, n = check_object("mnrf_field.o", "v_mfma_f32_16x16x4_f32", [
        (r"field_kernelILb[01]ELb0EE", fwd32), (r"field_kernelILb[01]ELb1EE", dict(fwd32, scratch_inside_max=4)),
        (r"field_bwd2?_kernel", grad32)])
    ok &= o and n >= 9
    # the D-NeRF object field (mnrf_dnerf.hip): the same hand-placed scheme over two networks in one launch
    o, n5 = check_object("mnrf_dnerf.o", "v_mfma_f32_16x16x4_f32", [(r"dnerf_kernel", fwd32)])
    ok &= o and n5 >= 4
    fwd16 = dict(min_counted=100, counted_re=r"s_waitcnt lgkmcnt\([24]\)", scratch_inside_max=0, scratch_total_max=0)
    grad16 = dict(fwd16, scratch_inside_max=400, scratch_total_max=600)
    # short conversion form, per 256-wide layer loop: 531 / 547 at 32 samples per wave (the long form: 723 / 739), 794 / 810 at 48
    # (1082 / 1098); the bounds leave 20 for a compiler's change of mind and lie 170 and 270 below the long form
    short32 = dict(layer_mfma=768, layer_valu_max=567)
    short48 = dict(layer_mfma=1152, layer_valu_max=830)
    o, n2 = check_object("mnrf_field_split.o", "v_mfma_f32_16x16x32_f16", [
        (r"4mnrf2h218field_split_kernel", dict(fwd16, **short32)),
        (r"field_split_kernel", fwd16),
        # the planes variants are the training default: the activation-gradient kernel keeps a handful of long-lived scalars in
        # scratch (9 reloads inside its streams since round 4; it was 161 while dL/dh8 was live through the colour branch, and that
        # cost 12 % of the kernel), the second-order kernel none
        (r"field_split_bwd_kernelILb1", dict(grad16, scratch_inside_max=12, scratch_total_max=40)),
        # round 5: with its plane stores woven into the GEMMs (6.13-6.18 against 6.26-6.30 ms per TotalLoss step) the store context
        # costs the second-order kernel 3 reloads inside its streams (scratch operations only make the counted vmcnt waits stricter)
        (r"field_split_bwd2_kernelILb1", dict(grad16, scratch_inside_max=6, scratch_total_max=100)),
        (r"field_split_bwd2?_kernel", grad16)])
    ok &= o and n2 >= 10
    # 48-samples-per-wave tuning (S = 3, forward only): the sigma-only kernel must not spill; the full kernel's heads spill a
    # few B operands (safe: vmcnt waits only get stricter; reported and bounded)
    o, n4 = check_object("mnrf_field_split3.o", "v_mfma_f32_16x16x32_f16", [
        # (h3l: the same five kernels with the long conversion form, kept for comparison -- every bound but the conversion's)
        (r"4mnrf3h3l.*field_split_kernelILb0ELb0ELb0ELb1", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", scratch_total_max=8)),
        (r"4mnrf3h3l.*field_split_kernel_(rgb_depth|blended)", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", scratch_total_max=8)),
        (r"4mnrf3h3l.*field_split_kernel", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)")),
        (r"field_split_kernelILb1ELb0", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", **short48)),        # one unit of read-ahead: the unit's wait is lgkmcnt(0)
        # the full kernel: ZERO scratch since round 3 (sample index and lane group recomputed from the execution-mask count),
        # also with the tile loop of the dynamic queue (every lane-derived value re-derived per tile through an opaque lane id).
        # Its ray-fused variant (FUSE): zero inside the network; the compositing wave at the end of a tile re-reads two
        # lane-derived values (the lane id behind __shfl_*) that hipcc hoists out of the tile loop: 2 stores per launch,
        # 5 loads per tile in one wave -- bounded
        (r"field_split_kernelILb0ELb0ELb0ELb0", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", **short48)),
        (r"field_split_kernelILb0ELb0ELb0ELb1", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", scratch_total_max=8, **short48)),
        # its rgb / depth variant (the last reflection level): the same network without the mirror head, the same bound
        (r"field_split_kernel_rgb_depth", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", scratch_total_max=8, **short48)),
        # its blended-level variant: the whole network (the mirror head in front of the colour branch), the same bound
        (r"field_split_kernel_blended", dict(fwd16, counted_re=r"s_waitcnt lgkmcnt\(0\)", scratch_total_max=8, **short48))])
    ok &= o and n4 >= 10
    if n < 9 or n2 < 10:
        print(f"expected >= 9 fp32 and >= 10 split kernels, found {n} and {n2}")
    # weight-gradient GEMMs: no hand-placed scheme, but a spill there is a 2x slowdown nobody would notice
    for sym, body in disassemble(os.path.join(CSRC, "mnrf_dw.o")).items():
        s = sum("scratch_" in l for l in body)
        if "dw_gemm" in sym:
            print(f"{sym}: {sum('v_mfma' in l for l in body)} MFMA, {s} scratch ops")
            ok &= s == 0
    # plane-fed weight-gradient GEMM (round 3): transposing LDS reads and LDS-DMA present, nothing spills
    for sym, body in disassemble(os.path.join(CSRC, "mnrf_dwp.o")).items():
        if "dwp_gemm" in sym:
            s = sum("scratch_" in l for l in body)
            tr = sum("ds_read_b64_tr_b16" in l for l in body)
            dma = sum("global_load_lds_dwordx4" in l for l in body)
            # the only VMEM loads of the kernel are its LDS-DMA tiles: the counted vmcnt waits of the ring assume it, and a vector
            # load of the (device-made) work plan in front of every job cost 35 us per launch in the first DEV build (round 5)
            vl = sum(bool(re.search(r"\bglobal_load_(dword|ushort|short|ubyte|sbyte)", l)) and "lds" not in l for l in body)
            print(f"{sym}: {sum('v_mfma' in l for l in body)} MFMA, {tr} ds_read_b64_tr_b16, {dma} LDS-DMA tiles, {s} scratch ops, "
                  f"{vl} vector loads")
            ok &= s == 0 and tr > 0 and dma > 0 and vl == 0
    if not ok:
        print("ISA CHECK FAILED")
        sys.exit(1)
    print("ISA check ok")


if __name__ == "__main__":
    main()
