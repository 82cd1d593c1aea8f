"""Pins from the reference itself: its tokenizer and image I/O, compiled
UNMODIFIED from the reference's sources (oracle/Makefile `ref`,
oracle/ref_harness.cpp -> oracle/_ref/libref_io.so), against the product's
own (librtx_host.so):

* the token stream and every scalar of each .ray fixture, and of edge-case
  texts, equal the product tokenizer's (Tokenizer.cpp:39-237, Token.cpp);
* readImage of every BMP / PNG fixture equals rtx_read_image byte for byte
  (bitmap.cpp:17-93, pngimage.cpp:195-216 with the image's own libpng 1.6);
* writeImage and rtx_write_image produce the same BMP bytes, and PNGs that
  both readers decode to the same pixels (pngimage.cpp:226-285).

Where the reference's sources are present the reference is asked directly,
and the record of its answers under tests/golden/ref_pins/
(tools/make_ref_pins.py) must say the same.  Where they are absent the record
stands in for it (tests/ref_pins.py), so the tests run everywhere."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import ref_pins as rp
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def ref():
    """the reference's library, or None where only the record is there"""
    return rp.load_ref() if rp.live() else None


@pytest.fixture(scope="module")
def pins():
    return rp.pins()


@pytest.fixture(scope="module")
def host(pkg):
    L = pkg.host_lib()
    L.rtx_host_tokens.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
    return L


_tokens = rp.tokens


def _ray_fixtures():
    out = sorted(glob.glob(os.path.join(GOLDEN, "**", "*.ray"), recursive=True))
    out += sorted(p for p in glob.glob(os.path.join(ROOT, "scenes", "*.ray")) if not p.endswith("dragon.ray"))
    return out


@pytest.fixture(scope="module")
def orc_tokens(pkg, orc):
    orc.lib(pkg)
    return orc.lib(pkg).oracle_tokens


def _recorded(table, path):
    """the record's entry for an input file, which must be the file recorded"""
    rel = os.path.relpath(path, ROOT)
    assert rel in table, f"{rel}: not in tests/golden/ref_pins/pins.json (tools/make_ref_pins.py records it)"
    e = table[rel]
    assert e["input_sha256"] == rp.file_sha(path), f"{rel} is not the file the record was taken from"
    return e


@pytest.mark.parametrize("path", _ray_fixtures(), ids=lambda p: os.path.relpath(p, ROOT))
def test_token_stream_matches_reference(ref, pins, host, orc_tokens, path):
    """Both tokenizers, the product's (parser.cpp) and the checker's own
    (oracle/parse_restated.cpp), against the reference's."""
    got, got_orc = _tokens(host.rtx_host_tokens, path), _tokens(orc_tokens, path)
    want_pin = _recorded(pins["tokens"], path)["tokens"]
    if ref is not None:
        want = _tokens(ref.ref_tokens, path)
        assert want[-1] == "EOF"
        assert got == want
        assert got_orc == want
        assert rp.token_pin(want) == want_pin  # the record is the reference's answer
    else:
        assert got[-1] == "EOF"
        assert rp.token_pin(got) == want_pin
        assert rp.token_pin(got_orc) == want_pin


EDGE_TEXTS = rp.EDGE_TEXTS


@pytest.mark.parametrize("name", list(EDGE_TEXTS))
def test_token_edge_cases_match_reference(ref, pins, host, orc_tokens, tmp_path, name):
    p = tmp_path / f"{name}.ray"
    p.write_bytes(EDGE_TEXTS[name].encode())
    e = pins["edge_tokens"][name]
    assert e["text"] == EDGE_TEXTS[name]
    if ref is not None:
        want = _tokens(ref.ref_tokens, str(p))
        assert e["tokens"] == want  # the record is the reference's answer
    else:
        want = e["tokens"]
    assert _tokens(host.rtx_host_tokens, str(p)) == want
    assert _tokens(orc_tokens, str(p)) == want


def _read(host, path):
    """rtx_read_image: (h, w, channels)"""
    w, h, ch = C.c_int32(), C.c_int32(), C.c_int32()
    if host.rtx_read_image(path.encode(), C.byref(w), C.byref(h), C.byref(ch), None, 0) != 0:
        return None
    out = np.zeros(w.value * h.value * ch.value, np.uint8)
    assert host.rtx_read_image(path.encode(), C.byref(w), C.byref(h), C.byref(ch), out.ctypes.data, out.size) == 0
    return out.reshape(h.value, w.value, ch.value)


_ref_read = rp.ref_read


def _image_fixtures():
    return sorted(p for p in glob.glob(os.path.join(GOLDEN, "**", "*.bmp"), recursive=True) +
                  glob.glob(os.path.join(GOLDEN, "**", "*.png"), recursive=True)
                  if os.path.dirname(p) != rp.PINS_DIR)  # (the record's own files: test_write_image_...)


@pytest.mark.parametrize("path", _image_fixtures(), ids=lambda p: os.path.relpath(p, GOLDEN))
def test_read_image_matches_reference(ref, pins, host, path):
    got = _read(host, path)
    want_pin = _recorded(pins["images"], path)["pixels"]
    assert want_pin is not None
    assert got is not None
    if ref is not None:
        want = _ref_read(ref, path)
        assert want is not None, ref.ref_last_error()
        assert got.shape == want.shape
        assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
        assert rp.image_pin(want) == want_pin  # the record is the reference's answer
    else:
        assert list(got.shape) == want_pin["shape"]
        assert rp.image_pin(got) == want_pin


@pytest.mark.parametrize("ext", [".bmp", ".png"])
@pytest.mark.parametrize("w,h", rp.WRITE_SIZES)
def test_write_image_matches_reference(ref, pins, host, tmp_path, ext, w, h):
    rgb = rp.write_input(w, h)
    e = pins["write"][rp.write_name(w, h, ext)]
    assert e["input_sha256"] == rp.image_pin(rgb)["sha256"]
    a, b = str(tmp_path / f"ref{ext}"), str(tmp_path / f"rtx{ext}")
    recorded_a = open(os.path.join(rp.PINS_DIR, rp.write_name(w, h, ext)), "rb").read()
    if ref is not None:
        assert ref.ref_write_image(a.encode(), w, h, rgb.ctypes.data) == 0
        if ext == ".bmp":  # (a PNG's bytes also depend on the zlib that packed it)
            # the record is what the reference wrote (up to the last row's
            # padding, which writeBMP reads from past its buffer: below)
            fa = open(a, "rb").read()
            n = len(fa) - (4 - w * 3 % 4) % 4
            assert len(recorded_a) == len(fa) and recorded_a[:n] == fa[:n]
    else:
        with open(a, "wb") as f:
            f.write(recorded_a)
    assert host.rtx_write_image(b.encode(), w, h, rgb.ctypes.data) == 0
    if ext == ".bmp":
        fa, fb = open(a, "rb").read(), open(b, "rb").read()
        assert len(fa) == len(fb)
        # byte for byte, except the last row's padding: writeBMP copies the
        # padded row length from the packed buffer (bitmap.cpp:137), i.e.
        # reads past its end there (undefined; decision U25: zeros)
        pad = (4 - w * 3 % 4) % 4
        n = len(fa) - pad
        assert fa[:n] == fb[:n]
        assert fb[n:] == bytes(pad)
    for path, key in ((a, "ref_reads_ref"), (b, "ref_reads_rtx")):
        hi = _read(host, path)
        if ref is not None:
            ri = _ref_read(ref, path)
            assert ri is not None and hi is not None and np.array_equal(hi, ri)
            assert rp.image_pin(ri) == e[key]  # the record is the reference's answer
        else:
            # (the reference's reading of the product's file was recorded on the
            # bytes the product wrote then: the same bytes for a BMP, which the
            # comparison above holds to the reference's; a PNG must decode to
            # the writer's buffer, as the reference read it — checked below)
            assert hi is not None and rp.image_pin(hi) == e[key]
        if ext == ".png":  # the buffer the writer was given
            assert np.array_equal(hi, rgb)
        # (readBMP compacts padded rows in place with out = in - offset, and
        # where the offset is 1 byte `out[1] = in[1]` overwrites in[0] before
        # `out[2] = in[0]` reads it (bitmap.cpp:76-90): such rows read back
        # with a wrong third channel — in the reference and here alike)
