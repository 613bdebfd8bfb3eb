"""Registers and scratch of every `tail16` instantiation, read from the gfx950 code-object metadata (no GPU needed).

tail16 is one 1024-thread workgroup per CU: 16 waves, four per SIMD, so a wave may have 512 / 4 = 128 vector registers.  The kernel
keeps per-wave constants resident in most of them; an edit that needs more does not fail to build, it spills to
scratch and costs speed silently.  One device-only compile of kernels_bf16.hip with the Makefile's HIPFLAGS (about 15 s), shared by
the tests of this module; skipped where there is no hipcc.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sr-for-cfd_amd", "csrc")
VGPR_LIMIT = 128     # 512 registers per SIMD lane / 4 waves per SIMD
INSTANTIATIONS = 14  # F16 x OUT (f32, bf16, f16) x SEG, and the two section-timer (PROF) ones


def _hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return cand if os.path.isfile(cand) and os.access(cand, os.X_OK) else None


def _makefile_hipflags():
    """HIPFLAGS of the default (non-DIAG) build, expanded by hand: CXXFLAGS + the offload architecture + the contraction switch."""
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = {}
    for name in ("ARCH", "CXXFLAGS", "HIPFLAGS"):
        m = re.search(r"^%s\s*[:?]?=\s*(.*)$" % name, text, re.M)
        assert m, name
        var[name] = m.group(1).strip()
    flags = var["HIPFLAGS"].replace("$(CXXFLAGS)", var["CXXFLAGS"]).replace("$(ARCH)", var["ARCH"])
    assert "$(" not in flags, flags
    return flags.split()


@pytest.fixture(scope="module")
def tail16_kernels(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc on this machine")
    flags = _makefile_hipflags()
    assert "--offload-arch=gfx950" in flags, flags
    out = tmp_path_factory.mktemp("tail16_listing") / "kernels_bf16.s"
    subprocess.run([hipcc] + flags + ["--cuda-device-only", "-S", "-o", str(out), "kernels_bf16.hip"], cwd=CSRC, check=True,
                   capture_output=True, text=True)
    text = out.read_text()
    meta = text[text.index(".amdgpu_metadata"):text.index(".end_amdgpu_metadata")]
    kernels = {}
    for block in re.split(r"^  - (?=\.)", meta, flags=re.M)[1:]:
        name = re.search(r"^\s*\.name:\s*(\S+)", block, re.M).group(1)
        if not re.match(r"_ZN5srcfd6tail16I", name):   # tail16<...>, not tail16s
            continue
        kernels[name] = {k: int(re.search(r"^\s*\.%s:\s*(\d+)" % k, block, re.M).group(1))
                         for k in ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "max_flat_workgroup_size")}
    return kernels


def test_every_instantiation_is_in_the_code_object(tail16_kernels):
    assert len(tail16_kernels) == INSTANTIATIONS, sorted(tail16_kernels)
    assert all(k["max_flat_workgroup_size"] == 1024 for k in tail16_kernels.values())


def test_registers_fit_four_waves_per_simd_without_scratch(tail16_kernels):
    for name, k in sorted(tail16_kernels.items()):
        print(name, k)
        assert k["vgpr_count"] <= VGPR_LIMIT, (name, k)
        assert k["private_segment_fixed_size"] == 0, (name, k)
        assert k["vgpr_spill_count"] == 0, (name, k)
