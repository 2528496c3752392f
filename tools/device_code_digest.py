"""A digest of the device code in a libnwe_hip.so, for comparing two builds ("device code unchanged"): for every gfx950 code
object, in link order, one line for its .note metadata and one line per kernel, sorted by name - symbol, size and sha256 of its
bytes in .text, sha256 of its 64-byte descriptor (<name>.kd in .rodata).  Two builds hold the same kernels exactly if
`diff` finds their outputs equal.  Whole code objects are NOT comparable: the compilation-unit id symbol (__hip_cuid_<hash>) is
derived from the source path and the options, so symbol and string tables change with a file name.

    python tools/device_code_digest.py [path/to/libnwe_hip.so] > digest.txt"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin/"   # as tools/check_m0.py


def digest(lib_path):
    lines = []
    sha = lambda b: hashlib.sha256(b).hexdigest()
    with tempfile.TemporaryDirectory() as tmp:
        shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
        subprocess.run([LLVM + "llvm-objdump", "--offloading", "lib.so"], cwd=tmp, check=True, capture_output=True)
        objects = sorted((n for n in os.listdir(tmp) if n.endswith("gfx950")), key=lambda n: [int(x) for x in re.findall(r"\d+", n)])
        for index, name in enumerate(objects):
            elf = open(os.path.join(tmp, name), "rb").read()
            out = subprocess.run([LLVM + "llvm-readelf", "-S", "-s", "-W", name], cwd=tmp, check=True, capture_output=True, text=True).stdout
            # section headers: [Nr] Name Type Address Off Size ...; symbols: Num: Value Size Type Bind Vis Ndx Name
            secs = {int(m[1]): (m[2], int(m[3], 16), int(m[4], 16), int(m[5], 16))
                    for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", out, re.M)}
            syms = {m[4]: (int(m[1], 16), int(m[2]), int(m[3]))
                    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+\S+\s+\S+\s+\S+\s+(\d+)\s+(\S+)$", out, re.M)}

            def data(symbol, section):
                value, size, ndx = syms[symbol]
                sec_name, addr, off, _ = secs[ndx]
                assert sec_name == section, (symbol, sec_name)
                return elf[off + value - addr:off + value - addr + size]

            note = next(s for s in secs.values() if s[0] == ".note")
            kernels = sorted(s[:-3] for s in syms if s.endswith(".kd"))
            lines.append(f"code object {index}: {len(kernels)} kernels, .note {note[3]} bytes {sha(elf[note[2]:note[2] + note[3]])}")
            for k in kernels:
                kd = data(k + ".kd", ".rodata")
                assert len(kd) == 64, (k, len(kd))
                lines.append(f"{k} {syms[k][1]} {sha(data(k, '.text'))} {sha(kd)}")
    return lines


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print("\n".join(digest(sys.argv[1] if len(sys.argv) > 1 else os.path.join(root, "nerf-workspaces-explorer_amd", "libnwe_hip.so"))))
