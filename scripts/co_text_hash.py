"""Hash the device code of each .hip unit, to show that a refactor left the
kernels' machine code alone.  Compiles device-only for RPGPU_ARCH with the
flags of redpanda_amd/build.py, unbundles the code object and prints
  unit  sha256(.text)  sha256(.rodata)  bytes(.text)
Compare two trees' outputs line by line; other ELF sections differ with the
path, so whole files are not comparable.  Usage:
  python scripts/co_text_hash.py [--tree DIR] [--units a.hip,b.hip] [-DFOO ...]"""
import hashlib
import os
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from redpanda_amd import build as B  # noqa: E402

args = sys.argv[1:]
tree, units = ROOT, [s for s in B.HIP_SOURCES if s != "rp_runtime.hip"]  # the runtime unit has no kernels
if "--tree" in args:
    i = args.index("--tree")
    tree = os.path.abspath(args[i + 1])
    del args[i:i + 2]
if "--units" in args:
    i = args.index("--units")
    units = args[i + 1].split(",")
    del args[i:i + 2]
inc, csrc = os.path.join(tree, "include"), os.path.join(tree, "redpanda_amd", "csrc")
llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(B._hipcc()))), "lib", "llvm", "bin")


def section(co, name):
    out = co + name
    B._run([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=" + name, co, out])
    with open(out, "rb") as f:
        return f.read()


def one(unit):
    with tempfile.TemporaryDirectory() as tmp:
        bundle, co = os.path.join(tmp, "u.hipfb"), os.path.join(tmp, "u.co")
        B._run([B._hipcc(), f"--offload-arch={B.ARCH}", "-O3", "-fPIC", "-std=c++17", "-I", inc, "-I", csrc, "-Wall",
                "-Wno-unused-function", "-Wno-unused-variable", "-Wno-unused-label"] + args
               + ["--offload-device-only", "--gpu-bundle-output", "-c", os.path.join(csrc, unit), "-o", bundle])
        B._run([os.path.join(llvm, "clang-offload-bundler"), "--unbundle", "--type=o", f"--targets=hipv4-amdgcn-amd-amdhsa--{B.ARCH}",
                "--input=" + bundle, "--output=" + co])
        text, ro = section(co, ".text"), section(co, ".rodata")
        return f"{unit:18s} {hashlib.sha256(text).hexdigest()}  {hashlib.sha256(ro).hexdigest()}  {len(text)}"


with ThreadPoolExecutor(min(8, int(os.environ.get("MAX_JOBS", "0") or 0) or 8)) as ex:
    for line in ex.map(one, units):
        print(line)
