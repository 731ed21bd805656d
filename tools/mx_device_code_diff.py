"""Byte comparison of the device code of two builds of the same HIP sources, per kernel.

    python tools/mx_device_code_diff.py OLD_DIR NEW_DIR > profiles/mx_host_launch_device_code.txt
    python tools/mx_device_code_diff.py --resources OLD_DIR NEW_DIR FILE... > profiles/mx_w16_resources.txt

OLD_DIR and NEW_DIR hold one plain gfx950 ELF per source, NAME.elf, compiled with the Makefile's flags plus
`--cuda-device-only --no-gpu-bundle-output -c`.  For every file the two builds must define the same function and kernel-descriptor
symbols, every symbol's bytes must be equal, and every kernel's metadata entry (registers, LDS, scratch, arguments) must be equal.  The
only symbol left out is __hip_cuid_*, whose name is a hash of the source text, and the only field left out is a kernel descriptor's
kernel_code_entry_byte_offset (bytes 16 .. 23 of the 64-byte NAME.kd): it is the distance from the descriptor to the kernel's code, which
moves whenever another kernel of the same file changes size.  A line per file, then a line per kernel template that differs, saying
in how many instances and in what (code, descriptor, metadata); exit status 1 on any difference.

--resources lists, for the named files (no extension) and every kernel whose name holds `decode`, `gemm` or `dgrad`, the two builds'
VGPRs (with AGPRs), SGPRs, LDS bytes and scratch bytes from the kernels' metadata, old -> new, and the waves per SIMD that the VGPRs
allow (512 registers per SIMD lane in steps of 8, at most 8 waves).  Exit status 1 where scratch is not 0, LDS differs or the new
build's VGPRs allow fewer waves."""
import hashlib
import os
import re
import subprocess
import sys

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def run(*a):
    return subprocess.run(a, check=True, capture_output=True, text=True).stdout


def sections(path):
    """index -> (address, file offset, size, type) from the section headers"""
    out = {}
    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S*)\s+(\S+)\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run(f"{LLVM}/llvm-readelf", "-S", "-W", path), re.M):
        out[int(m.group(1))] = (int(m.group(4), 16), int(m.group(5), 16), int(m.group(6), 16), m.group(3))
    return out


def symbols(path):
    """name -> bytes of every FUNC symbol (code) and OBJECT symbol (kernel descriptors, constants)"""
    blob = open(path, "rb").read()
    sec = sections(path)
    out = {}
    for line in run(f"{LLVM}/llvm-readelf", "--symbols", "-W", path).splitlines():
        f = line.split()
        if len(f) < 8 or f[3] not in ("FUNC", "OBJECT") or not f[6].isdigit() or f[7].startswith("__hip_cuid_"):
            continue
        addr, size, (s_addr, s_off, _, s_type) = int(f[1], 16), int(f[2]), sec[int(f[6])]
        data = b"" if s_type == "NOBITS" else blob[s_off + addr - s_addr:s_off + addr - s_addr + size]
        if f[7].endswith(".kd") and len(data) == 64:
            data = data[:16] + bytes(8) + data[24:]  # kernel_code_entry_byte_offset
        out[f[7]] = data
    return out


def metadata(path):
    """kernel name -> its amdhsa.kernels entry, as text"""
    notes = run(f"{LLVM}/llvm-readelf", "--notes", path)
    out = {}
    for entry in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):notes.index("amdhsa.target:")])[1:]:
        out[re.search(r"\.name:\s+(\S+)", entry).group(1)] = entry
    return out


def main(old_dir, new_dir):
    bad = 0
    for name in sorted(f for f in os.listdir(new_dir) if f.endswith(".elf")):
        old, new = os.path.join(old_dir, name), os.path.join(new_dir, name)
        so, sn, mo, mn = symbols(old), symbols(new), metadata(old), metadata(new)
        diff = sorted(set(so) ^ set(sn)) + [k for k in so if k in sn and so[k] != sn[k]] + sorted(set(mo) ^ set(mn)) + [k for k in mo if k in mn and mo[k] != mn[k]]
        code = hashlib.sha256(b"".join(sn[k] for k in sorted(sn))).hexdigest()[:16]
        whole = hashlib.sha256(open(old, "rb").read()).digest() == hashlib.sha256(open(new, "rb").read()).digest()
        print(f"{name[:-4] + '.hip':22s} kernels {len(mn):3d}  symbols {len(sn):3d}  symbol bytes {sum(map(len, sn.values())):7d}  sha256[:16] {code}  "
              f"whole file {'equal' if whole else 'differs (__hip_cuid_* only)' if not diff else 'differs'}  {'IDENTICAL' if not diff else 'DIFFERENT'}")
        bad += bool(diff)
        what = {}  # kernel template -> {what differs: instances}
        for k in set(diff):
            kind = "metadata" if k in mo and k in mn and mo[k] != mn[k] and not (k in so and k in sn and so[k] != sn[k]) else \
                "descriptor" if k.endswith(".kd") else "code" if k in so and k in sn else "present in one build only"
            kd = k[:-3] if k.endswith(".kd") else k
            m = re.match(r"_ZN3bie(\d+)", kd)  # bie::NAME<...>: the length-prefixed identifier after the namespace
            short = kd[m.end():m.end() + int(m.group(1))] if m else kd
            what.setdefault(short, {}).setdefault(kind, set()).add(kd)
            if kind == "code" and k in mo and k in mn and mo[k] != mn[k]:
                what[short].setdefault("metadata", set()).add(kd)
        for short in sorted(what):
            print(f"    {short}: " + ", ".join(f"{kind} of {len(v)} instance{'s' * (len(v) > 1)}" for kind, v in sorted(what[short].items())))
    return 1 if bad else 0


def resources(old_dir, new_dir, files):
    field = lambda e, k: int(re.search(rf"\.{k}:\s+(\d+)", e).group(1))
    waves = lambda e: min(8, 512 // max(8, (field(e, "vgpr_count") + field(e, "agpr_count") + 7) // 8 * 8))
    bad = 0
    print(f"{'kernel':78s} {'VGPR':>10s} {'SGPR':>10s} {'LDS':>14s} {'scratch':>8s} {'waves':>6s}")
    for name in files:
        mo, mn = metadata(os.path.join(old_dir, name + ".elf")), metadata(os.path.join(new_dir, name + ".elf"))
        for k in sorted(mn):
            if not re.search("decode|gemm|dgrad", k):
                continue
            o, n = mo[k], mn[k]
            col = lambda key: f"{field(o, key)} -> {field(n, key)}"
            ok = field(n, "private_segment_fixed_size") == 0 and field(o, "group_segment_fixed_size") == field(n, "group_segment_fixed_size") and waves(n) >= waves(o)
            bad += not ok
            print(f"{name + ' ' + k:78s} {col('vgpr_count'):>10s} {col('sgpr_count'):>10s} {col('group_segment_fixed_size'):>14s} "
                  f"{col('private_segment_fixed_size'):>8s} {waves(o)} -> {waves(n)}{'' if ok else '  FAILS'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(resources(sys.argv[2], sys.argv[3], sys.argv[4:]) if sys.argv[1] == "--resources" else main(sys.argv[1], sys.argv[2]))
