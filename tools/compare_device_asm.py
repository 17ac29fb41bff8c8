"""Is the gfx950 device code of two source trees the same?  For host-only refactors.
    python tools/compare_device_asm.py <other checkout> [file.hip ...]      (default: every csrc/*.hip that differs between the two trees)
Compiles each file of both trees with -save-temps (as tools/kernel_regs.py does) and compares the *gfx950*.s files function by function: the same set of
kernel symbols and, per function, identical instruction text.  Symbol order, debug / file lines and the function index inside local labels (.LBB<n>_) are ignored.
Exit status 1 when anything else differs."""
import filecmp, glob, os, re, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def functions(root, name, tmp):
    d = os.path.join(tmp, name.replace(".", "_")); os.makedirs(d)
    csrc = os.path.join(root, "comfy-rvc_amd", "csrc")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{root}/include", f"-I{csrc}", "-save-temps", "-c",
                    os.path.join(csrc, name), "-o", "x.o"], cwd=d, stderr=subprocess.DEVNULL, check=True)
    txt = open(glob.glob(os.path.join(d, "*gfx950*.s"))[0]).read()
    out = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        body = [re.sub(r"\.L(BB|JTI|tmp|func_begin|func_end)\d+_?", r".L\1_", ln.split(";")[0].rstrip()) for ln in m.group(2).split("\n")]
        out[m.group(1)] = "\n".join(ln for ln in body if ln.strip() and not ln.strip().startswith((".loc", ".file", ".cfi", ".p2align")))
    return out, set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))


def main():
    other = os.path.abspath(sys.argv[1])
    rel = os.path.join("comfy-rvc_amd", "csrc")
    names = sys.argv[2:] or sorted(os.path.basename(p) for p in glob.glob(os.path.join(HERE, rel, "*.hip"))
                                   if not (os.path.exists(os.path.join(other, rel, os.path.basename(p))) and filecmp.cmp(p, os.path.join(other, rel, os.path.basename(p)), False)))
    bad = total = 0
    for n in names:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            (fa, ka), (fb, kb) = functions(other, n, ta), functions(HERE, n, tb)
        differ = sorted(f for f in fa if f in fb and fa[f] != fb[f])
        ok = set(fa) == set(fb) and ka == kb and not differ
        total += len(kb); bad += not ok
        print(f"{n:24s} kernels {len(ka):3d} / {len(kb):3d}  {'identical' if ok else 'DIFFERENT'}", *(differ[:3] + sorted(set(fa) ^ set(fb))[:3]))
    print(f"{total} kernels in {len(names)} files, {bad} files differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
