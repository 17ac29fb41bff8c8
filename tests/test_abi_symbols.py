"""CPU: the C-ABI library builds, loads, and exports every symbol include/rvc_hip.h declares (no compute without a GPU)."""
import os
import re

from conftest import ROOT


def _declared_symbols(experiments=False):
    """Symbols of the product ABI (experiments=False) or of the `#ifdef RVC_EXPERIMENTS` section at the end of the header."""
    hdr = open(os.path.join(ROOT, "include", "rvc_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"#ifdef RVC_EXPERIMENTS(.*?)#endif", hdr, flags=re.S)
    assert m, "the header keeps its instrumentation hooks in an RVC_EXPERIMENTS section"
    part = m.group(1) if experiments else hdr[:m.start()] + hdr[m.end():]
    return sorted(set(re.findall(r"\b(rvc_[a-z0-9_]+)\s*\(", part)))


def test_library_exports_every_declared_symbol():
    from comfy_rvc_amd import _lib
    syms = _declared_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(_lib.lib, s), f"{s} declared in include/rvc_hip.h but not exported"
        assert s in _lib.SIGNATURES, f"{s} has no ctypes signature in _lib.py"
    assert set(_lib.SIGNATURES) == set(syms)
    exp = _declared_symbols(experiments=True)
    assert set(_lib.EXPERIMENT_SIGNATURES) == set(exp) and all(e.startswith("rvc_debug_") for e in exp)
    assert not any(s.startswith("rvc_debug_") for s in syms)


def test_product_library_has_no_experiment_hooks_and_only_documented_knobs():
    """The product build (csrc/Makefile, no -DRVC_EXPERIMENTS) exports no rvc_debug_* symbol and carries no environment-variable name beyond the documented
    knobs of INTEGRATION.md ("Run-time knobs"): experiment switches are compiled to their defaults and their names never reach the binary."""
    import subprocess
    from comfy_rvc_amd import _lib
    if os.environ.get("RVC_HIP_LIB"):
        return                                                       # a variant build is loaded on purpose
    assert not _lib.has_experiments
    blob = open(_lib.LIB_PATH, "rb").read()
    names = set(n.decode() for n in re.findall(rb"RVC_[A-Z0-9_]{2,}", blob))
    names = {n for n in names if not n.startswith(("RVC_HIP_CHECK", "RVC_REQUIRE", "RVC_TRY", "RVC_CATCH"))}
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = doc[doc.index("## Run-time knobs"):]
    sec = sec[:sec.index("\n## ", 5)] if "\n## " in sec[5:] else sec
    documented = set(re.findall(r"`(RVC_[A-Z0-9_]+)`", sec))
    assert names <= documented, f"undocumented RVC_ strings in the product library: {sorted(names - documented)}"
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    assert "rvc_debug_" not in exported


def test_no_cpu_fallback_without_gpu():
    import ctypes as C
    import torch
    from comfy_rvc_amd import _lib
    if torch.cuda.is_available():
        return
    h = C.c_void_p()
    assert _lib.lib.rvc_ctx_create(0, C.byref(h)) != 0
    assert b"device" in _lib.lib.rvc_last_error().lower()


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "comfy-rvc_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(d, f)


def test_pair_arithmetic_knob():
    """RVC_H2 is the documented environment form of rvc_set_pair_arithmetic's initial mode (no GPU needed: the getter touches no device)."""
    import subprocess
    import sys
    code = "from comfy_rvc_amd import _lib; a = _lib.lib.rvc_get_pair_arithmetic(); _lib.check(_lib.lib.rvc_set_pair_arithmetic(1 - a)); print(a, _lib.lib.rvc_get_pair_arithmetic())"
    for env, want in (({}, "1 0"), ({"RVC_H2": "0"}, "0 1"), ({"RVC_H2": "1"}, "1 0")):
        e = dict(os.environ); e.pop("RVC_H2", None); e.update(env)
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e)
        assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == want, (env, out.stdout, out.stderr[-500:])


CSRC = os.path.join(ROOT, "comfy-rvc_amd", "csrc")
PER_FILE_FLAGS = {"attention_dma": "-amdgpu-mfma-vgpr-form=1", "audio_fx": "-ffp-contract=off"}


def _compile_commands(*make_args):
    """{stem: command} of `make -n -B` in csrc/ (nothing is compiled): every compile command names exactly one .hip, every .hip exactly one command."""
    import subprocess
    out = subprocess.run(["make", "-n", "-B", "-C", CSRC, *make_args], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-500:]
    cmds = {}
    for line in out.stdout.splitlines():
        if " -c " not in line:
            continue
        stems = re.findall(r"(?<![\w/.-])(\w+)\.hip\b", line)
        assert len(stems) == 1 and stems[0] not in cmds, line
        cmds[stems[0]] = line
    present = sorted(f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(cmds) == present, (sorted(set(present) - set(cmds)), sorted(set(cmds) - set(present)))
    return cmds


def test_one_source_list_for_the_product_and_the_variant_builds():
    """csrc/Makefile is the only list of the .hip files and of their per-file flags: the plain build and a VARIANT build compile every .hip of csrc/ exactly
    once, the variant with -DRVC_EXPERIMENTS and its EXTRA flags into variants/, the plain one with neither; tools/build_variant.sh names no source file."""
    plain, variant = _compile_commands(), _compile_commands("VARIANT=t", "EXTRA=-DXYZ")
    for stem in plain:
        p, v = plain[stem].split(), variant[stem].split()
        assert "-DRVC_EXPERIMENTS" not in p and "-DXYZ" not in p and not any("variants/" in w for w in p), plain[stem]
        assert p[p.index("-o") + 1] == stem + ".o"
        assert "-DRVC_EXPERIMENTS" in v and "-DXYZ" in v and v[v.index("-o") + 1] == f"variants/obj_t/{stem}.o", variant[stem]
        for cmd in (p, v):
            for owner, flag in PER_FILE_FLAGS.items():
                assert (flag in cmd) == (stem == owner), (stem, flag)
    script = open(os.path.join(ROOT, "tools", "build_variant.sh")).read()
    assert not [s for s in plain if re.search(rf"\b{s}\b", script)]


def test_shared_device_helpers_have_one_definition():
    """The helpers the kernel files share exist once under csrc/ (comments do not count): the -DRVC_CONV_TIMING conditional (phase_timing.h), the immediate
    vmcnt wait, the branch-free GELU (by its first constant) and the buffer-to-LDS DMA call."""
    src = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(CSRC, f)).read()
            src[f] = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert len(src) > 30

    def files_with(pattern):
        return [f for f, t in src.items() if re.search(pattern, t, flags=re.M)]

    assert files_with(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif)\b[^\n]*\bRVC_CONV_TIMING\b") == ["phase_timing.h"]
    assert len(files_with(re.escape("s_waitcnt vmcnt(%0)"))) == 1
    assert len(files_with(re.escape("0.3275911f"))) == 1
    assert sum(len(re.findall(r"raw_ptr_buffer_load_lds\s*\(", t)) for t in src.values()) == 1
