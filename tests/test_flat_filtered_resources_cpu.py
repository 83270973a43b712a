"""The resource baseline of the filtered flat search's kernels (no GPU needed).  They are built into a library of their own,
jvector_amd/libjvector_hip_fa.so (jvector_amd/csrc/k_flat_accept.hip), so their baseline is a fixture of its own,
tests/golden/kernel_resources_flat_accept.json, held to the rules tests/test_bq_compact_resources_cpu.py holds the compaction library
to — no figure of a kernel's metadata note above the recorded one, no kernel without a line — and the scan and map kernels use neither
spills nor scratch at all.  The reader of the code objects' notes is restated here.  Metadata fields only; no instruction is looked at."""
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
LIB = os.path.join(ROOT, "jvector_amd", "libjvector_hip_fa.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_resources_flat_accept.json")
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size")
SCAN_AND_MAP = ("flat_accept_sums_kernel", "flat_accept_scan_kernel", "flat_accept_write_kernel", "flat_accept_map_kernel")
LIST_ADC = 10   # adc_mq_list_kernel<VSF, SLCH, R>: two slice widths x (R = 4 for three similarity functions, R = 8 for two)
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


def test_every_kernel_is_within_its_recorded_resources(resources):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(resources) == sorted(want)
    for k in SCAN_AND_MAP:
        assert len([name for name in resources if k in name]) == 1, k
    assert len([name for name in resources if "adc_mq_list_kernel" in name]) == LIST_ADC
    assert len(resources) == len(SCAN_AND_MAP) + LIST_ADC
    worse = ["%s: %s %d > %d" % (k, fld, got[fld], want[k][fld]) for k, got in sorted(resources.items()) for fld in FIELDS if got[fld] > want[k][fld]]
    assert not worse, "kernels above their recorded resources:\n" + "\n".join(worse)


def test_the_scan_and_map_kernels_spill_nothing(resources):
    for k, got in resources.items():
        if any(s in k for s in SCAN_AND_MAP):
            assert (got["vgpr_spill_count"], got["sgpr_spill_count"], got["private_segment_fixed_size"]) == (0, 0, 0), (k, got)


def test_the_recorded_list_adc_kernels_spill_nothing_either():
    with open(FIXTURE) as f:
        want = json.load(f)
    for k, v in want.items():
        assert (v["vgpr_spill_count"], v["sgpr_spill_count"], v["private_segment_fixed_size"]) == (0, 0, 0), k
        assert v["vgpr_count"] <= 128, k     # what a workgroup of 1024 threads may hold


def test_the_engine_library_links_the_filtered_search_library_next_to_itself():
    import jvector_amd
    assert os.path.dirname(jvector_amd.LIB_PATH) == os.path.dirname(LIB) and os.path.exists(LIB)
    raw = ctypes.CDLL(jvector_amd.LIB_PATH)          # resolves libjvector_hip_fa.so through its $ORIGIN run path
    assert hasattr(raw, "jv_hip_search_flat_filtered")
