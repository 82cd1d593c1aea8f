"""What the reference itself answers, live or recorded (shared by
tests/test_ref_pins.py, tests/test_traceui_adapter.py and
tools/make_ref_pins.py).

Where the reference sources are present (REF_SRC), its tokenizer and image
I/O are compiled unmodified into oracle/_ref/libref_io.so (oracle/Makefile
`ref`) and asked directly; the tests then also check that the record under
tests/golden/ref_pins/ says the same, so the record cannot go stale unseen.
Where they are absent, the record answers: what those same functions returned
when tools/make_ref_pins.py ran them — token streams and decoded images as
sha256 + size (keyed by the input file's own sha256, so a changed input is
noticed), the edge-case token streams in full, and the image files the
reference's writeImage wrote."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np

from conftest import GOLDEN, ROOT

def _ref_src():
    """where the recipe (oracle/Makefile, `REF ?= ...`) looks for the reference's sources"""
    if os.environ.get("REF"):
        return os.environ["REF"]
    with open(os.path.join(ROOT, "oracle", "Makefile")) as f:
        for ln in f:
            if ln.startswith("REF ") and "?=" in ln:
                return ln.split("?=", 1)[1].strip()
    raise RuntimeError("oracle/Makefile names no REF")


REF_SRC = _ref_src()
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libref_io.so")
PINS_DIR = os.path.join(GOLDEN, "ref_pins")
PINS_JSON = os.path.join(PINS_DIR, "pins.json")
WRITE_SIZES = [(1, 1), (3, 2), (37, 19), (64, 64)]

# edge cases of the scanner: comments, quoted identifiers, aliases, scalars
# atof reads partially ('1-2', '1e', '--3', '.'), identifiers with '-',
# reserved words without names in getNameForToken, syntax errors
EDGE_TEXTS = {
    "comments": "SBT-raytracer 1.0\n// line comment\n/* block\n comment */ camera { fov = 30; }\n",
    "scalars": "1 -2 .5 -.25 1e3 1e-3 1e 1-2 --3 . 3.14159265358979323846 1e400 -0 007\n",
    "idents": 'foo _bar a-b-c "quoted name" "with space" colour polymesh gennormals fov x1y2\n',
    "punct": "( ) { } , = ;\n",
    "no_newline_at_eof": "sphere { material = { diffuse = (0.1, 0.2, 0.3); } }",
    "crlf": "SBT-raytracer 1.0\r\ncamera {\r\n position = (1,2,3);\r\n}\r\n",
    "unterminated_string": 'name = "oops\n',
    "unterminated_comment": "camera /* never closed\n",
    "bad_char": "camera { position = (1, 2, 3) } @\n",
    "slash_alone": "camera / 3\n",
    "empty": "",
}


def live():
    return os.path.isdir(REF_SRC)


def load_ref():
    """the reference's tokenizer + image I/O (live only)"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, capture_output=True)
    L = C.CDLL(REF_LIB)
    L.ref_tokens.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
    L.ref_read_image.argtypes = [C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                 C.c_void_p, C.c_int64]
    L.ref_write_image.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_void_p]
    L.ref_last_error.restype = C.c_char_p
    return L


def pins():
    with open(PINS_JSON) as f:
        return json.load(f)


def tokens(fn, path):
    n = C.c_int64()
    assert fn(path.encode(), None, 0, C.byref(n)) == 0
    b = C.create_string_buffer(n.value)
    assert fn(path.encode(), b, n.value, C.byref(n)) == 0
    return b.value.decode(errors="replace").splitlines()


def ref_read(ref, path):
    """readImage: the pixels (h, w, channels).  readBMP's vector is height *
    padded-row bytes long with the pixels packed at the front (bitmap.cpp:
    57-91) — what TextureMap::getPixelAt reads, (x + y * width) * 3
    (material.cpp:128-132); readPNG's is exactly rowbytes * height."""
    w, h, n = C.c_int32(), C.c_int32(), C.c_int64()
    if ref.ref_read_image(path.encode(), C.byref(w), C.byref(h), C.byref(n), None, 0) != 0:
        return None
    out = np.zeros(n.value, np.uint8)
    assert ref.ref_read_image(path.encode(), C.byref(w), C.byref(h), C.byref(n), out.ctypes.data, out.size) == 0
    npx = w.value * h.value
    ch = 3 if path.lower().endswith(".bmp") else n.value // npx
    return out[: npx * ch].reshape(h.value, w.value, ch)


def file_sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def token_pin(lines):
    """a token stream as the record holds it"""
    return {"n": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


def image_pin(px):
    """a decoded image as the record holds it (None: the reader refused the file)"""
    if px is None:
        return None
    return {"shape": list(px.shape), "sha256": hashlib.sha256(np.ascontiguousarray(px).tobytes()).hexdigest()}


def write_input(w, h):
    """the buffer the writers are given"""
    return np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)


def write_name(w, h, ext):
    return f"write_{w}x{h}{ext}"


def adapter_sources_sha():
    """the adapter, its checker and the option parsing behind the recorded
    rows of tests/test_traceui_adapter.py"""
    h = hashlib.sha256()
    for p in ("include/rtx_traceui.h", "include/rtx.h", "tests/native/traceui_adapter_check.cpp",
              "cs378hgraphics-raytracer_amd/csrc/host/cli_opts.h"):
        with open(os.path.join(ROOT, p), "rb") as f:
            h.update(f.read())
    return h.hexdigest()
