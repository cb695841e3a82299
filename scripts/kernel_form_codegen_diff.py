#!/usr/bin/env python3
"""Compare the gfx950 code of abm_kernels.hip and abm_kernels_pe.hip between two trees: the one before the mapping kernels
took their form as one template argument (abm_kernel_form.hpp) and the one after.

For each tree and each of the two files, beforehand:
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --offload-device-only --no-gpu-bundle-output \
        -Rpass-analysis=kernel-resource-usage -c FILE.hip -o DIR/FILE.co 2> DIR/FILE.remarks
then:  kernel_form_codegen_diff.py OLD_DIR NEW_DIR > profiles/kernel_form_codegen_diff.txt

The mapping from old to new symbol names is OLD_TO_NEW below: an old name's template arguments, read off its mangled
name, are the fields of a form, and the new name carries that form's id (PeForm::id / SeForm::id)."""
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
FILES = ("abm_kernels", "abm_kernels_pe")
EXPECT = {"abm_kernels": 20, "abm_kernels_pe": 36}
SE_BIT = 1 << 31


def pe_id(phase, big, is_long, timed, coop, rec, text, bam, wps):
    return phase | big << 2 | is_long << 3 | timed << 4 | coop << 5 | rec << 6 | text << 7 | bam << 8 | wps << 9


def se_id(timed, coop, rec, bam, is_long, wps):
    return SE_BIT | timed | coop << 1 | rec << 2 | bam << 3 | is_long << 4 | wps << 9


def template_args(sym):
    return [int(v) for v in re.findall(r"L[bi](\d+)E", sym)]


def OLD_TO_NEW(sym):
    """the new name of an old kernel symbol (other kernels keep theirs)"""
    if sym.startswith("_ZN3abm13map_pe_kernelI"):
        big, timed, coop, wps, lng, phase, rec, text, bam = template_args(sym)
        return "_ZN3abm13map_pe_kernelILj%dEEEvNS_6PeArgsE" % pe_id(phase, big, lng, timed, coop, rec, text, bam, wps)
    if sym.startswith("_ZN3abm13map_se_kernelI"):
        timed, coop, rec = template_args(sym)
        return "_ZN3abm13map_se_kernelILj%dEEEvNS_6SeArgsE" % se_id(timed, coop, rec, 0, 0, 5)
    if sym.startswith("_ZN3abm17map_se_bam_kernelI"):
        coop, rec = template_args(sym)
        return "_ZN3abm13map_se_kernelILj%dEEEvNS_6SeArgsE" % se_id(0, coop, rec, 1, 0, 5)
    if sym == "_ZN3abm18map_se_long_kernelENS_6SeArgsE":
        return "_ZN3abm13map_se_kernelILj%dEEEvNS_6SeArgsE" % se_id(0, 0, 0, 0, 1, 1)
    return sym


def kernels(co):
    out = subprocess.run([LLVM + "llvm-readelf", "--dyn-syms", co], check=True, capture_output=True, text=True).stdout
    return sorted(l.split()[7] for l in out.splitlines() if " FUNC " in l)


def resources(remarks):
    res, cur = {}, None
    for line in open(remarks):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).partition(": ")
        if key == "Function Name":
            cur = res.setdefault(val.strip(), {})
        elif cur is not None and key.strip() != "Dynamic Stack":
            cur[key.strip()] = val.strip()
    return res


def rodata(co):
    """(address, bytes) of the code object's .rodata"""
    out = subprocess.run([LLVM + "llvm-readelf", "-S", "-W", co], check=True, capture_output=True, text=True).stdout
    f = re.search(r"\] \.rodata\s+PROGBITS\s+([0-9a-f]+) ([0-9a-f]+) ([0-9a-f]+)", out)
    addr, off, size = (int(v, 16) for v in f.groups())
    with open(co, "rb") as fh:
        fh.seek(off)
        return addr, fh.read(size)


def disassembly(co, rename):
    """{symbol: [instruction lines]}: addresses dropped, symbol names through `rename`, padding between kernels dropped.
    A kernel finds its constant tables by s_getpc_b64 + s_add_u32 with the distance from itself to .rodata, which depends
    on where the linker put the kernel; the distance is replaced by the 16 bytes it points at.  A long jump is made the same way:
    its distance becomes the target's offset from the kernel's start"""
    out = subprocess.run([LLVM + "llvm-objdump", "-d", co], check=True, capture_output=True, text=True).stdout
    ro_addr, ro = rodata(co)
    body, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^([0-9a-f]+) <(.*)>:$", line)
        if m:
            start, cur = int(m.group(1), 16), body.setdefault(rename(m.group(2)), [])
            continue
        if cur is None or not line.strip() or line.strip() == "...":
            continue
        ins, _, comment = line.partition("//")
        ins = ins.strip()
        lit = re.match(r"s_add_u32 (s\d+), \1, 0x([0-9a-f]+)$", ins)
        if lit and cur and cur[-1].startswith("s_getpc_b64"):
            at = (int(comment.split(":")[0], 16) + int(lit.group(2), 16)) % (1 << 32)
            where = ".rodata: " + ro[at - ro_addr:at - ro_addr + 16].hex() if ro_addr <= at < ro_addr + len(ro) else "this kernel + 0x%x" % (at - start)
            ins = "s_add_u32 %s, %s, <%s>" % (lit.group(1), lit.group(1), where)
        target = re.search(r"<([^>+]+)(\+0x[0-9a-f]+)?>", comment)
        cur.append(ins + (" -> %s%s" % (rename(target.group(1)), target.group(2) or "") if target else ""))
    for lines in body.values():  # (alignment padding after a kernel's last instruction)
        while lines and lines[-1] in ("s_nop 0", "s_code_end"):
            lines.pop()
    return body


def main(old_dir, new_dir):
    differ = []
    total = 0
    for f in FILES:
        old_k, new_k = kernels(f"{old_dir}/{f}.co"), kernels(f"{new_dir}/{f}.co")
        print(f"{f}.hip: {len(old_k)} kernels before, {len(new_k)} after (expected {EXPECT[f]})")
        assert len(old_k) == len(new_k) == EXPECT[f]
        assert sorted(OLD_TO_NEW(k) for k in old_k) == new_k, "the renamed old kernels are not the new kernels"
        old_r, new_r = resources(f"{old_dir}/{f}.remarks"), resources(f"{new_dir}/{f}.remarks")
        old_d, new_d = disassembly(f"{old_dir}/{f}.co", OLD_TO_NEW), disassembly(f"{new_dir}/{f}.co", lambda s: s)
        for k in old_k:
            n = OLD_TO_NEW(k)
            same_r, same_d = old_r[k] == new_r[n], old_d[n] == new_d[n]
            total += 1
            r = new_r[n]
            print(f"  {k}\n    -> {n}\n    VGPRs {r['VGPRs']} AGPRs {r['AGPRs']} SGPRs {r['TotalSGPRs']} scratch {r['ScratchSize [bytes/lane]']} "
                  f"spills {r['SGPRs Spill']}/{r['VGPRs Spill']} occupancy {r['Occupancy [waves/SIMD]']} LDS {r['LDS Size [bytes/block]']}; "
                  f"{len(new_d[n])} instructions; resources {'equal' if same_r else 'DIFFER'}, instruction stream {'identical' if same_d else 'DIFFERS'}")
            if not (same_r and same_d):
                differ.append((k, old_r[k], new_r[n]))
    print(f"\n{total} kernels compared, {len(differ)} differ")
    for k, a, b in differ:
        print(f"  {k}\n    before {a}\n    after  {b}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
