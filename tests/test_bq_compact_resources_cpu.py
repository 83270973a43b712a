"""The resource baseline of the BQ compaction kernels (no GPU needed).  They are built into a library of their own,
jvector_amd/libjvector_hip_bqc.so (jvector_amd/csrc/k_bq_compact.hip), so their baseline is a fixture of its own,
tests/golden/kernel_resources_bq_compact.json, held to the rule tests/test_kernel_resources_cpu.py holds the engine library to — no
figure of a kernel's metadata note above the recorded one, no kernel without a line — and to one more: none of them spills or uses
scratch at all.  The reader of the code objects' notes is restated here.  Metadata fields only; no instruction is looked at."""
import ctypes
import json
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "jvector_amd", "libjvector_hip_bqc.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_resources_bq_compact.json")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
KERNELS = ("rank_sums", "rank_scan", "rank_write", "rows", "bq_rows", "fill_bits")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for d in (os.path.join(rocm, "llvm", "bin"), os.path.join(rocm, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return shutil.which(name)


def code_objects(fatbin):
    """the device ELF images of a .hip_fatbin section: one uncompressed offload bundle per translation unit"""
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
                out.append(fatbin[at + off: at + off + size])
        at = fatbin.find(BUNDLE_MAGIC, pos)
    return out


def kernel_resources(lib):
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
        for i, image in enumerate(objs):
            assert image[:4] == b"\x7fELF", "a compressed or unknown code object"
            co = os.path.join(tmp, "co%d.elf" % i)
            with open(co, "wb") as f:
                f.write(image)
            notes = subprocess.check_output([readelf, "--notes", co], text=True)
            for block in re.split(r"\n\s*- \.", notes):   # one "- .agpr_count: ..." block per kernel
                name = re.search(r"^\s*\.?symbol:\s*'?([^'\n]+?)'?\s*$", block, re.M)
                if not name or not name.group(1).endswith(".kd"):
                    continue
                vals = {}
                for fld in FIELDS:
                    m = re.search(r"^\s*\.?" + fld + r":\s*(\d+)\s*$", block, re.M)
                    assert m, (name.group(1), fld)
                    vals[fld] = int(m.group(1))
                res[name.group(1)[:-3]] = vals
    return res


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(LIB):
        import __graft_entry__ as G
        G.build()
    return kernel_resources(LIB)


def test_every_compaction_kernel_is_within_its_recorded_resources(resources):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(resources) == sorted(want)
    for k in KERNELS:
        assert len([name for name in resources if "bq_compact_%s_kernel" % k in name]) == 1, k
    assert len(resources) == len(KERNELS)
    worse = ["%s: %s %d > %d" % (k, fld, got[fld], want[k][fld]) for k, got in sorted(resources.items()) for fld in FIELDS if got[fld] > want[k][fld]]
    assert not worse, "kernels above their recorded resources:\n" + "\n".join(worse)


def test_no_compaction_kernel_spills(resources):
    for k, got in resources.items():
        assert (got["vgpr_spill_count"], got["sgpr_spill_count"], got["private_segment_fixed_size"]) == (0, 0, 0), (k, got)


def test_the_engine_library_links_the_compaction_library_next_to_itself():
    import jvector_amd
    assert os.path.dirname(jvector_amd.LIB_PATH) == os.path.dirname(LIB)
    raw = ctypes.CDLL(jvector_amd.LIB_PATH)          # resolves libjvector_hip_bqc.so through its $ORIGIN run path
    assert hasattr(raw, "jv_hip_bq_builder_compact")
