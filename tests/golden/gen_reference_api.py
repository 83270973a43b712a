"""Generates tests/golden/reference_vector_api.json: the declarations of the reference's vector API that the Java shim
(jvector-native-hip/) extends or names, so that tests/test_java_shim_cpu.py can check the shim without a reference checkout.

Recorded, per base type the shim overrides (VectorUtilSupport, PanamaVectorUtilSupport, VectorizationProvider): every method
declaration as (name, parameter types, return type), extracted by the test's own parser; per class the shim names: its
declaration modifiers.
Run:  python tests/golden/gen_reference_api.py /path/to/jvector-checkout
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from test_java_shim_cpu import _java_methods, _strip_comments  # noqa: E402

VECTOR = "src/main/java/io/github/jbellis/jvector/vector"
BASE_TYPES = [("jvector-base", "VectorUtilSupport"), ("jvector-twenty", "PanamaVectorUtilSupport"),
              ("jvector-base", "VectorizationProvider")]
CLASSES = [("jvector-twenty", "PanamaVectorUtilSupport"), ("jvector-native", "MemorySegmentVectorFloat"),
           ("jvector-native", "MemorySegmentByteSequence"), ("jvector-native", "MemorySegmentVectorProvider")]


def _source(ref, module, cls):
    with open(os.path.join(ref, module, VECTOR, cls + ".java")) as fh:
        return fh.read()


def main(ref):
    out = {"methods": {}, "classes": {}}
    for module, cls in BASE_TYPES:
        out["methods"][cls] = [[name, list(types), ret] for (name, types), ret in sorted(_java_methods(_source(ref, module, cls)).items())]
    for module, cls in CLASSES:
        m = re.search(r"((?:\b(?:public|protected|private|final|abstract|static|sealed)\s+)*)class\s+" + cls + r"\b",
                      _strip_comments(_source(ref, module, cls)))
        out["classes"][cls] = {"modifiers": m.group(1).split()}
    path = os.path.join(HERE, "reference_vector_api.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/gen_reference_api.py /path/to/jvector-checkout")
    main(sys.argv[1])
