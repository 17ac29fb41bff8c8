"""CPU: the host scaffolding the model graphs share: the two-pass arena driver and the zero-margin block guard under AddressSanitizer + UBSan in a
host-only program, and the absence of the per-model copies they replaced."""
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "comfy-rvc_amd", "csrc")


def test_graph_helpers_host_program_is_clean_under_sanitizers(tmp_path):
    """tests/host/graph_helpers_main.cpp defines Arena::ensure / release over malloc / free.  arena_passes: the graph runs twice, ensure sees the dry pass's peak, a
    throw in either pass leaves dry == false.  ZeroedBlock: stale on first use, not on an identical second use, again after a change of base, generation, bytes or
    either key and after reset()."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on the build machine")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "graph_helpers")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
           f"-I{ROOT}/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", os.path.join(ROOT, "tests", "host", "graph_helpers_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode} (100 = a check failed)\n{r.stderr[-3000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_per_model_copies_of_the_graph_scaffolding_are_gone():
    """One driver loop (arena_passes), one guard (ZeroedBlock), one tap helper, and no column-softmax route behind the text encoder's attention."""
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and p.endswith((".hip", ".h"))}
    models = {n: t for n, t in src.items() if re.fullmatch(r"model_\w+\.hip", n)}
    assert len(models) == 5
    for name, text in models.items():
        assert "pass < 2" not in text and not re.search(r"for \(int pass\b", text), f"a two-pass driver loop in {name}"
        assert "img_base" not in text, f"an img_base member in {name}"
        assert "auto tap" not in text, f"a tap lambda in {name}"
        assert "hipMemsetAsync(A.base" not in text, f"a hand-written image guard in {name}"
    for name, text in src.items():
        assert "softmax_cols" not in text, f"softmax_cols in {name}"
    assert sum(t.count("A.ensure(A.peak)") for t in src.values()) == 1
    assert sum(len(re.findall(r"\battention_split\(s,", t)) for n, t in src.items() if n.startswith("model_")) == 1, "one split-resident encoder layer"
