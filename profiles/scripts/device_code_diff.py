"""Is the device code of two trees the same?  For a change that is meant to touch the host side only.

    python profiles/scripts/device_code_diff.py OTHER_TREE [THIS_TREE] [--out profiles/call_args/device_code.txt]

Every .hip source of the library is compiled in both trees to a plain gfx950 code object (the product's flags plus
--offload-device-only --no-gpu-bundle-output), and three things are compared byte for byte: the .text section (the
kernels), the .rodata section (the kernel descriptors: argument sizes, register and LDS allocation) and the dump of the
notes (per kernel: registers, scratch, LDS, the argument layout).  Whole files are not compared: they differ in a symbol
per translation unit that hashes the source.  One line per source; the exit status is 1 if anything differs.  No GPU."""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cutadapt_amd import build  # noqa: E402

LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")


def code_object(tree, src, out_dir):
    obj = os.path.join(out_dir, src + ".co")
    subprocess.run([build._hipcc(), f"--offload-arch={build.ARCH}", "-O3", "-std=c++17", "-fPIC", "-x", "hip",
                    "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(tree, "cutadapt_amd", "csrc", src), "-o", obj],
                   check=True)
    parts = {}
    for sec in (".text", ".rodata"):
        raw = obj + sec
        subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", f"--only-section={sec}", obj, raw], check=True)
        with open(raw, "rb") as fh:
            parts[sec] = fh.read()
    parts["notes"] = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, capture_output=True).stdout
    return parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("other_tree")
    ap.add_argument("this_tree", nargs="?", default=ROOT)
    ap.add_argument("--out")
    a = ap.parse_args()
    sources = [s for s in build.SOURCES if s.endswith(".hip")]
    lines, same = [], True
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = {}
        for label, tree in (("other", a.other_tree), ("this", a.this_tree)):
            os.makedirs(os.path.join(tmp, label))
            for src in sources:
                jobs[label, src] = pool.submit(code_object, os.path.abspath(tree), src, os.path.join(tmp, label))
        for src in sources:
            o, t = jobs["other", src].result(), jobs["this", src].result()
            cols = []
            for part in (".text", ".rodata", "notes"):
                eq = o[part] == t[part]
                same = same and eq and len(t[part]) > 0
                cols.append(f"{part} {'identical' if eq else 'DIFFERENT'} ({len(t[part])} B, sha256 {hashlib.sha256(t[part]).hexdigest()[:12]})")
            lines.append(f"{src:18s} " + "  ".join(cols))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
