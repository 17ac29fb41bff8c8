"""CPU: who owns device memory on the host side of csrc/ ("Ownership").  The owners themselves under AddressSanitizer + UBSan in a host-only
program, null handles at the C ABI, and the absence of the hand-written free lists the owners replaced."""
import ctypes as C
import glob
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "comfy-rvc_amd", "csrc")


def test_owners_host_program_is_clean_under_sanitizers(tmp_path):
    """tests/host/dev_owners_main.cpp defines dev_alloc / dev_upload / dev_free over malloc / free and counts live allocations: moves, vector growth, a view
    outliving nothing, `= {}` over an aggregate of owners.  Exit status 0 = nothing leaked; ASan / UBSan (linked statically) report double frees and the like."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("sanitizer runs belong on the build machine")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "dev_owners")
    cmd = [os.path.join(rocm, "llvm", "bin", "clang++"), "-std=c++17", "-x", "c++", "-D__HIP_PLATFORM_AMD__", f"-I{rocm}/include", f"-I{CSRC}",
           f"-I{ROOT}/include", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g", os.path.join(ROOT, "tests", "host", "dev_owners_main.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, f"exit {r.returncode} (live allocations, or 100 = a check failed)\n{r.stderr[-3000:]}"
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


NULL_HANDLE_ERRORS = [
    "rvc_hubert_set_tensor", "rvc_rmvpe_set_tensor", "rvc_synth_set_tensor", "rvc_crepe_set_tensor", "rvc_mdx23_set_tensor",
    "rvc_hubert_finalize", "rvc_rmvpe_finalize", "rvc_synth_finalize", "rvc_crepe_finalize", "rvc_mdx23_finalize",
    "rvc_hubert_forward", "rvc_rmvpe_forward", "rvc_crepe_forward", "rvc_mdx23_forward", "rvc_mdx23_demix", "rvc_rmvpe_decode",
    "rvc_index_search", "rvc_index_blend",
    "rvc_conv1d_plan_run", "rvc_conv1d_plan_pair_run", "rvc_conv1d_plan_pair_split_run", "rvc_conv1d_plan_resblock_run",
    "rvc_vc_segment", "rvc_vc_segment_window", "rvc_vc_segment_feats", "rvc_vc_segment_feats_window",
    "rvc_synth_infer", "rvc_synth_infer_window", "rvc_synth_infer_window_halo",
]
DESTROYS = ["rvc_hubert_destroy", "rvc_rmvpe_destroy", "rvc_synth_destroy", "rvc_crepe_destroy", "rvc_mdx23_destroy", "rvc_index_destroy",
            "rvc_conv1d_plan_destroy", "rvc_ctx_destroy"]


def _all_null(argtypes):
    """A null / zero value per parameter: with every pointer null nothing can reach a HIP call."""
    out = []
    for t in argtypes:
        if t in (C.c_float, C.c_double):
            out.append(t(0.0))
        elif t in (C.c_int, C.c_int64, C.c_uint, C.c_size_t):
            out.append(t(0))
        else:
            out.append(None)
    return out


SECOND_HANDLE = {"rvc_vc_segment", "rvc_vc_segment_window", "rvc_conv1d_plan_pair_run", "rvc_conv1d_plan_pair_split_run"}   # (handle, handle, ...)


@pytest.mark.parametrize("name", NULL_HANDLE_ERRORS)
def test_null_handle_is_an_error_not_a_crash(name):
    """First every argument null; then only the handle null (each handle in turn where there are two) and every other pointer a valid host buffer: the call must
    still be refused, which it can only be by the check of the handle itself.  That check comes first, so the buffers are never read."""
    from comfy_rvc_amd import _lib
    _, argtypes = _lib.SIGNATURES[name]
    fn = getattr(_lib.lib, name)
    calls = [_all_null(argtypes)]
    dummy = C.create_string_buffer(256)
    for null_at in ((0, 1) if name in SECOND_HANDLE else (0,)):
        args = _all_null(argtypes)
        for i, v in enumerate(args):
            if v is None and i != null_at:
                args[i] = C.cast(dummy, argtypes[i]) if argtypes[i] is not C.c_char_p else b"x"
        calls.append(args)
    for args in calls:
        assert fn(*args) != 0, f"{name} with a null handle returned success"
        assert _lib.lib.rvc_last_error(), f"{name} with a null handle left no message"


def test_destroy_of_null_is_a_no_op():
    from comfy_rvc_amd import _lib
    assert sorted(DESTROYS) == sorted(n for n in _lib.SIGNATURES if n.endswith("_destroy"))
    for name in DESTROYS:
        assert getattr(_lib.lib, name)(None) == 0, name


def test_hand_written_free_lists_are_gone():
    """Device memory is freed by its owners' destructors: no per-struct free function, no free_(), hipFree only where dev_free, the scratch pool and Arena live,
    and the single-op entry points allocate through DevBuf."""
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and p.endswith((".hip", ".h"))}
    assert len(src) > 30
    gone = ["free_()", "synth_free", "hubert_free", "rmvpe_free", "cbr_free", "crepe_free", "mdx23_free", "tfc_free", "scale_free"]
    for name, text in src.items():
        for g in gone:
            assert g not in text, f"{g} in {name}"
        if name != "conv_mfma.hip":
            assert "hipFree(" not in text, f"hipFree in {name}"
    assert sum(len(re.findall(r"conv_layer_free\(", t)) for t in src.values()) <= 1
    assert "hipMalloc(" not in src["rvc_api.hip"]
    assert not re.search(r"catch \(\.\.\.\) \{[^}]*throw; \}", src["rvc_api.hip"]), "a catch that only cleans up and rethrows"
