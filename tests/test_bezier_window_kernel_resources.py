"""Registers and scratch of the window forms' two kernels, read from the built library (host, no GPU).

bc_seed_window_kernel (csrc/bezier_certify.hpp) holds the polygon of one axis and the left part of a cut in registers, 2 x 13 doubles =
52 VGPRs, as bc_split_kernel does; its loops have constant bounds so that nothing is indexed at run time.  A change that makes an index
dynamic does not fail to build: the arrays move to scratch memory and the kernel only gets slower.  So two numbers are pinned: no
scratch, and at most 128 VGPRs (four waves per SIMD; DESIGN.md section 4 has the count of the build that was measured).

The numbers are taken from the kernel metadata exactly as tests/test_nn_kernel_resources.py takes them, with the same tools; the test
skips where those are not installed.  It reads two numbers per kernel and searches no instructions."""
import os
import re
import subprocess

import pytest

from pointcloudtraj_amd import build as B

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
KERNELS = ("bc_window_kernel", "bc_seed_window_kernel")


def llvm_tool(name):
    import shutil
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "lib", "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{kernel: (private_segment_fixed_size, vgpr_count)}"""
    tools = {n: llvm_tool(n) for n in ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")}
    if not all(tools.values()):
        pytest.skip("ROCm LLVM tools not found: " + ", ".join(n for n, p in tools.items() if not p))
    so = os.path.join(B.LIB, "libpct_engine.so")
    assert os.path.exists(so), "build the library first"
    tmp = tmp_path_factory.mktemp("fatbin")
    section = str(tmp / "hip_fatbin.bin")
    subprocess.run([tools["llvm-objcopy"], "--dump-section", ".hip_fatbin=" + section, so, os.devnull], check=True)
    data = open(section, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    assert starts, "no offload bundle in .hip_fatbin"
    out = {}
    for k, s in enumerate(starts):
        bundle, obj = str(tmp / f"bundle{k}.bin"), str(tmp / f"gfx950_{k}.o")
        with open(bundle, "wb") as f:
            f.write(data[s:starts[k + 1] if k + 1 < len(starts) else len(data)])
        subprocess.run([tools["clang-offload-bundler"], "--unbundle", "--type=o", "--targets=" + TARGET, "--input=" + bundle, "--output=" + obj], check=True)
        notes = subprocess.run([tools["llvm-readelf"], "--notes", obj], check=True, capture_output=True, text=True).stdout.splitlines()
        for i, ln in enumerate(notes):
            m = re.match(r"\s*\.name:\s+_ZN3pct\d+(" + "|".join(KERNELS) + r")E\S*\s*$", ln)
            if not m:
                continue
            got = {}
            for nx in notes[i + 1:]:
                f = re.match(r"\s*\.(private_segment_fixed_size|vgpr_count|wavefront_size):\s+(\d+)\s*$", nx)
                if f:
                    got[f.group(1)] = int(f.group(2))
                    if f.group(1) == "wavefront_size":
                        break
            assert "private_segment_fixed_size" in got and "vgpr_count" in got, (m.group(1), got)
            out[m.group(1)] = (got["private_segment_fixed_size"], got["vgpr_count"])
    return out


def test_both_kernels_are_there_without_scratch_and_within_128_vgprs(kernels):
    assert sorted(kernels) == sorted(KERNELS), sorted(kernels)
    for name, (scratch, vgprs) in sorted(kernels.items()):
        print(name, "scratch", scratch, "VGPRs", vgprs)
        assert scratch == 0, f"{name} spills: {scratch} bytes of scratch per lane"
        assert vgprs <= 128, f"{name}: {vgprs} VGPRs"
