"""Byte comparison of the device code of two builds of the same HIP sources, per kernel.

    python tools/mx_device_code_diff.py OLD_DIR NEW_DIR > profiles/mx_host_launch_device_code.txt

OLD_DIR and NEW_DIR hold one plain gfx950 ELF per source, NAME.elf, compiled with the Makefile's flags plus
`--cuda-device-only --no-gpu-bundle-output -c`.  For every file the two builds must define the same function and kernel-descriptor
symbols, every symbol's bytes must be equal, and every kernel's metadata entry (registers, LDS, scratch, arguments) must be equal.  The
only symbol left out is __hip_cuid_*, whose name is a hash of the source text.  A line per file; exit status 1 on any difference."""
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
        out[f[7]] = b"" if s_type == "NOBITS" else blob[s_off + addr - s_addr:s_off + addr - s_addr + size]
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
              f"whole file {'equal' if whole else 'differs (__hip_cuid_* only)' if not diff else 'differs'}  {'IDENTICAL' if not diff else 'DIFFERENT: ' + ' '.join(diff)}")
        bad += bool(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
