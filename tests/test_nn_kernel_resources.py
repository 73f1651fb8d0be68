"""Registers and scratch of the dense NN batch kernel, read from the built library (host, no GPU).

nn_grid_coop_kernel is built for a fixed number of waves per SIMD (kernels.hpp nn_coop_waves): 512 VGPRs per lane of a SIMD make 72 the
ceiling for 7 waves and 64 for 8.  A build that needs one register more does not fail: the compiler spills to scratch memory or splits the
nine record loads of stage 0 into several flights, and the kernel only gets slower.  That has decided three attempts at 8 waves without
anybody seeing it in a test, so the two numbers are pinned here: no scratch in any instantiation, and a VGPR count within the ceiling of
the occupancy the instantiation ships with.

The numbers come from the kernel metadata of the gfx950 code object inside libpct_engine.so's .hip_fatbin section (one offload bundle per
translation unit), taken out with the llvm-objcopy, clang-offload-bundler and llvm-readelf of the ROCm LLVM directory; the test skips
where those are not installed.  It reads two numbers per kernel and searches no instructions.
"""
import os
import re
import shutil
import subprocess

import pytest

from pointcloudtraj_amd import build as B

MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"

VGPR_CEILING = {7: 72, 8: 64}


def shipped_waves(count, narrow, block):
    """waves per SIMD of nn_grid_coop_kernel<COUNT, NARROW, BLOCK> as shipped (kernels.hpp nn_coop_waves): 7 for every instantiation --
    8 was built for <false, true, .> at 64 VGPRs without scratch and measured slower (profiles/r08_ab_unpacked_waves.txt)"""
    return 7


def llvm_tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "llvm", "bin"),
              os.path.join(os.path.dirname(os.path.realpath(B.HIPCC)), "..", "lib", "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{mangled name: (private_segment_fixed_size, vgpr_count)} of every nn_grid_coop_kernel in the library"""
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
        # a kernel's entry lists its keys in alphabetical order: .name, .private_segment_fixed_size, ..., .vgpr_count, ..., .wavefront_size
        for i, ln in enumerate(notes):
            m = re.match(r"\s*\.name:\s+(\S*nn_grid_coop_kernel\S*)\s*$", ln)
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


def instantiation(name):
    m = re.search(r"nn_grid_coop_kernelILb([01])ELb([01])ELi(\d+)EE", name)
    assert m, name
    return bool(int(m.group(1))), bool(int(m.group(2))), int(m.group(3))


def test_every_instantiation_is_there(kernels):
    assert sorted(instantiation(n) for n in kernels) == sorted((c, n, b) for c in (False, True) for n in (False, True) for b in (128, 256)), sorted(kernels)


def test_no_scratch(kernels):
    for name, (scratch, vgprs) in sorted(kernels.items()):
        print(instantiation(name), "scratch", scratch, "VGPRs", vgprs)
    for name, (scratch, _) in kernels.items():
        assert scratch == 0, f"{instantiation(name)} spills: {scratch} bytes of scratch per lane"


def test_vgprs_within_the_occupancy_that_ships(kernels):
    for name, (_, vgprs) in kernels.items():
        inst = instantiation(name)
        waves = shipped_waves(*inst)
        assert vgprs <= VGPR_CEILING[waves], f"{inst}: {vgprs} VGPRs, the ceiling for {waves} waves per SIMD is {VGPR_CEILING[waves]}"
