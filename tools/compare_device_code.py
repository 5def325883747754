#!/usr/bin/env python3
"""Device code of two checkouts, kernel by kernel: `compare_device_code.py OLD NEW` (no GPU needed).

Every source of each checkout's _build.SRCS is compiled with the product flags minus -fPIC -shared, plus -S
--cuda-device-only, and the assembly is cut into one text per kernel: the function body from its label to .Lfunc_end and
its .amdhsa_kernel block, without `;` comments and __hip_cuid_ lines, .LBB<n>_ written as .LBB_ and the kernel's own symbol
as KERNEL.  Kernels are keyed by their demangled name with template arguments and without the parameter list, so moving a
kernel to another file, or its argument struct to another namespace, leaves its key alone.  Prints the kernels that differ
(a kernel found under another key with the same text counts as renamed), diffs sources present on both sides as whole files,
and exits 1 if any code differs."""
import difflib
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile


def load_build(root):
    spec = importlib.util.spec_from_file_location("_build_" + str(abs(hash(root))), os.path.join(root, "simplegaussiansplat_tk71_amd", "_build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def clean(text):
    lines = (re.sub(r"\s*;.*", "", ln).rstrip() for ln in text.split("\n") if "__hip_cuid_" not in ln)
    return re.sub(r"\.LBB\d+_", ".LBB_", "\n".join(ln for ln in lines if ln.strip()))


def device_code(root, tmp):
    """({kernel key: text}, {source basename: whole cleaned assembly})"""
    b = load_build(root)
    flags = [f for f in b.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    cxxfilt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    kernels, files = {}, {}
    for src in b.SRCS:
        out = os.path.join(tmp, os.path.basename(src) + ".s")
        res = subprocess.run([b.find_hipcc(), *flags, "-I", b.INCLUDE, "-S", "--cuda-device-only", "-o", out, src], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr[-2000:]
        text = clean(open(out).read())
        files[os.path.basename(src)] = text
        for sym in re.findall(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
            body = re.search(r"^%s:\n.*?(?=^\.Lfunc_end\d+:)" % re.escape(sym), text, re.M | re.S).group(0)
            desc = re.search(r"^\s*\.amdhsa_kernel %s\n.*?\.end_amdhsa_kernel" % re.escape(sym), text, re.M | re.S).group(0)
            name = subprocess.run([cxxfilt, sym], capture_output=True, text=True, check=True).stdout.strip()
            depth, i = 0, len(name)
            while name.endswith(")") and (depth or i == len(name)):  # cut the parameter list: back to the `(` that opens it
                i -= 1
                depth += (name[i] == ")") - (name[i] == "(")
            key = re.sub(r"^void ", "", name[:i])
            assert key not in kernels, key
            kernels[key] = (body + desc).replace(sym, "KERNEL").replace(sym[2:], "KERNEL")
    return kernels, files


def main(old_root, new_root):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        (ka, fa), (kb, fb) = device_code(old_root, ta), device_code(new_root, tb)
    bad = 0
    for key in sorted(set(ka) & set(kb)):
        if ka[key] != kb[key]:
            bad += 1
            print("DIFFERS  " + key)
            print("\n".join(list(difflib.unified_diff(ka[key].split("\n"), kb[key].split("\n"), "old", "new", lineterm="", n=1))[:60]))
    gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    for key in gone:
        twins = [k for k in new if kb[k] == ka[key]]
        print("RENAMED  %s -> %s (same code)" % (key, twins[0]) if twins else "ONLY OLD %s" % key)
        bad += not twins
        new = [k for k in new if k not in twins[:1]]
    for key in new:
        bad += 1
        print("ONLY NEW " + key)
    for name in sorted(set(fa) & set(fb)):
        if fa[name] != fb[name]:
            bad += 1
            print("FILE DIFFERS  " + name)
    print("%d kernels old, %d new, %d sources on both sides: %s" % (len(ka), len(kb), len(set(fa) & set(fb)), "%d differences" % bad if bad else "identical"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])))
