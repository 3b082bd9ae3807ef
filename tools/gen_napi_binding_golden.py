"""Generate tests/golden/napi_binding.json: what the Node binding
(lodestar_amd/napi/index.js and lodestar_amd/napi/bgv_addon.c) makes of a seeded corpus.

The file pins two layers.  The JS layer runs every exported helper of index.js and both
verifier classes over a stand-in `addon` object: per encoder result the keys in order and
per array its constructor, length and SHA-256, the merging tables, every refusal's text,
and per verifier run the addon methods called with the digest of what they received, every
call's outcome and the metrics.  The addon layer links a second copy of bgv_addon.c against
tools/bgv_record_stub.c (as libbgv.so in a temporary directory) and records, for every
exported function, what the library saw, the result object, and every refusal of every
reader with the exception's constructor and text.  tools/napi_binding_golden.js is the
Node side; tests/test_napi_binding_golden.py replays record() and compares it with the file.

Needs node and node_api.h, neither the real library nor a GPU.  Rerun it only when the
binding's behaviour is meant to change:

    python tools/gen_napi_binding_golden.py
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import build as B  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "napi_binding.json")
NODE = shutil.which("node")


def available() -> bool:
    return NODE is not None and bool(B.NODE_INCLUDE)


def record() -> dict:
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tools", "bgv_record_stub.c"), "-o", os.path.join(tmp, "libbgv.so")])
        addon = B.build_addon(force=True, lib_dir=tmp, out=os.path.join(tmp, "bgv.node"))
        log = os.path.join(tmp, "calls.log")
        env = {**os.environ, "BGV_RECORD_LOG": log, "UV_THREADPOOL_SIZE": "16"}
        env.pop("BGV_RECORD_FAIL", None)
        r = subprocess.run([NODE, os.path.join(ROOT, "tools", "napi_binding_golden.js"), addon, log],
                           capture_output=True, text=True, timeout=300, env=env)
        if r.returncode != 0:
            raise RuntimeError(r.stdout[-2000:] + r.stderr[-4000:])
        return json.loads(r.stdout)


def dumps(rec: dict) -> str:
    """one line per case, so that a regenerated file diffs by case"""
    def line(v):
        return json.dumps(v, separators=(",", ":"))

    parts = []
    for section in sorted(rec):
        v = rec[section]
        if isinstance(v, dict):
            body = ",\n".join(f"  {line(k)}:{line(v[k])}" for k in sorted(v))
            parts.append(f"{line(section)}:{{\n{body}\n}}")
        else:
            parts.append(f"{line(section)}:{line(v)}")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main():
    if not available():
        sys.exit("node or node_api.h not found")
    text = dumps(record())
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {len(text)} bytes")


if __name__ == "__main__":
    main()
