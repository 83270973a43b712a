"""A resource baseline for every kernel of the built library (no GPU needed): the registers a kernel takes, the registers it spills
and its scratch bytes decide its occupancy and what its hot loops pay, and a change in a shared header (gs_body.h) moves them in
kernels nobody meant to touch — the fused rerank once took the builder's compacted pair kernels from 0 to 95 spilled VGPRs and was
only caught by a full benchmark run.

For every kernel of jvector_amd/libjvector_hip.so the four figures of its code object's metadata note — vgpr_count, vgpr_spill_count,
sgpr_spill_count, private_segment_fixed_size — may not EXCEED the value recorded in tests/golden/kernel_resources.json (lower is
fine; record the new figures then:  python tests/test_kernel_resources_cpu.py --write).  A kernel that is not in the fixture fails
too: a new kernel gets its line when it is added.  Metadata fields only; no instruction is looked at."""
import json
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jvector_amd", "libjvector_hip.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_resources.json")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def code_objects(fatbin):
    """the device ELF images of a .hip_fatbin section: one uncompressed offload bundle per translation unit, back to back"""
    out = []
    at = fatbin.find(BUNDLE_MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", fatbin, at + len(BUNDLE_MAGIC))
        pos = at + len(BUNDLE_MAGIC) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", fatbin, pos)
            triple = fatbin[pos + 24: pos + 24 + tl].decode()
            pos += 24 + tl
            if triple.startswith("hip") and size > 0:
                out.append((triple, fatbin[at + off: at + off + size]))
        at = fatbin.find(BUNDLE_MAGIC, pos)
    return out


def kernel_resources(lib=LIB):
    """{kernel symbol: {field: value}} from the metadata notes of every code object in the library"""
    objcopy, readelf = _tool("llvm-objcopy"), _tool("llvm-readelf")
    assert objcopy and readelf, "llvm-objcopy / llvm-readelf (the ROCm tree's LLVM tools) are needed to read the code objects' notes"
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.check_call([objcopy, "--dump-section", ".hip_fatbin=" + fat, lib, os.path.join(tmp, "unused.so")])
        with open(fat, "rb") as f:
            objs = code_objects(f.read())
        assert objs, "no device code object in " + lib
        for i, (triple, image) in enumerate(objs):
            assert image[:4] == b"\x7fELF", ("a compressed or unknown code object", triple)
            co = os.path.join(tmp, "co%d.elf" % i)
            with open(co, "wb") as f:
                f.write(image)
            notes = subprocess.check_output([readelf, "--notes", co], text=True)
            # the note is printed as YAML: one "- .agpr_count: ..." block per kernel, keys in alphabetical order
            for block in re.split(r"\n\s*- \.", notes):
                name = re.search(r"^\s*\.?symbol:\s*'?([^'\n]+?)'?\s*$", block, re.M)
                if not name or not name.group(1).endswith(".kd"):
                    continue
                vals = {}
                for fld in FIELDS:
                    m = re.search(r"^\s*\.?" + fld + r":\s*(\d+)\s*$", block, re.M)
                    assert m, (name.group(1), fld)
                    vals[fld] = int(m.group(1))
                key = name.group(1)[:-3]
                assert key not in res or res[key] == vals, ("one kernel, two code objects, different figures", key)
                res[key] = vals
    return res


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(LIB):
        import __graft_entry__ as G
        G.build()
    return kernel_resources()


def test_no_kernel_exceeds_its_recorded_resources(resources):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert len(resources) > 50
    missing = sorted(k for k in resources if k not in want)
    assert not missing, "kernels without a recorded baseline (python tests/test_kernel_resources_cpu.py --write): %s" % missing[:5]
    worse = []
    for k, got in sorted(resources.items()):
        for fld in FIELDS:
            if got[fld] > want[k][fld]:
                worse.append("%s: %s %d > %d" % (k, fld, got[fld], want[k][fld]))
    assert not worse, "kernels above their recorded resources:\n" + "\n".join(worse)


def test_the_plain_traversal_kernel_is_leaner_than_the_general_one(resources):
    """graph_search_ubr_plain_kernel<VSF, 6> (k_gsearch_ubr_plain.hip) exists for every similarity and spills less, with less scratch,
    than graph_search_ubr_kernel<VSF, 6, false>, the general kernel it is chosen over (the template arguments are read off the
    mangled names)"""
    for vsf in (0, 1, 2):
        gen = [v for k, v in resources.items() if re.search(r"graph_search_ubr_kernelILi%dELi6ELb0EE" % vsf, k)]
        pln = [v for k, v in resources.items() if re.search(r"graph_search_ubr_plain_kernelILi%dELi6EE" % vsf, k)]
        assert len(gen) == 1 and len(pln) == 1, (vsf, len(gen), len(pln))
        for fld in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert pln[0][fld] < gen[0][fld], (vsf, fld, pln[0][fld], gen[0][fld])


if __name__ == "__main__":
    r = kernel_resources(sys.argv[2] if len(sys.argv) > 2 else LIB)
    if len(sys.argv) > 1 and sys.argv[1] == "--write":
        with open(FIXTURE, "w") as f:
            json.dump(r, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", len(r), "kernels to", FIXTURE)
    else:
        json.dump(r, sys.stdout, indent=0, sort_keys=True)
