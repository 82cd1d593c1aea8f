#!/usr/bin/env python3
"""Record what the reference's own tokenizer and image I/O answer
(oracle/_ref/libref_io.so, oracle/Makefile `ref`: needs the reference's
sources) into tests/golden/ref_pins/, for tests/test_ref_pins.py and
tests/test_traceui_adapter.py to use where the reference is absent:

  pins.json            token streams and decoded images as sha256 + size,
                       edge-case token streams in full, the rows of
                       tests/native/traceui_adapter_check.cpp
  write_<w>x<h>.bmp    the files the reference's writeImage wrote for the
  write_<w>x<h>.png    tests' seeded buffers

Run after build() (the generated scenes must exist) whenever a fixture, the
edge-case texts or the adapter change; the tests compare the record with the
live reference wherever that is present."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_pins as rp  # noqa: E402
import test_ref_pins as trp  # noqa: E402
import test_traceui_adapter as tta  # noqa: E402
from conftest import load_package  # noqa: E402


def main():
    if not rp.live():
        sys.exit(f"make_ref_pins: no reference sources at {rp.REF_SRC}")
    ref = rp.load_ref()
    host = load_package().host_lib()
    os.makedirs(rp.PINS_DIR, exist_ok=True)
    out = {"tokens": {}, "edge_tokens": {}, "images": {}, "write": {}}
    for path in trp._ray_fixtures():
        out["tokens"][os.path.relpath(path, ROOT)] = {"input_sha256": rp.file_sha(path),
                                                     "tokens": rp.token_pin(rp.tokens(ref.ref_tokens, path))}
    with tempfile.TemporaryDirectory() as tmp:
        for name, text in rp.EDGE_TEXTS.items():
            p = os.path.join(tmp, f"{name}.ray")
            with open(p, "wb") as f:
                f.write(text.encode())
            out["edge_tokens"][name] = {"text": text, "tokens": rp.tokens(ref.ref_tokens, p)}
        for path in trp._image_fixtures():
            out["images"][os.path.relpath(path, ROOT)] = {"input_sha256": rp.file_sha(path),
                                                         "pixels": rp.image_pin(rp.ref_read(ref, path))}
        for w, h in rp.WRITE_SIZES:
            for ext in (".bmp", ".png"):
                rgb = rp.write_input(w, h)
                a = os.path.join(rp.PINS_DIR, rp.write_name(w, h, ext))
                b = os.path.join(tmp, "rtx" + ext)
                assert ref.ref_write_image(a.encode(), w, h, rgb.ctypes.data) == 0
                assert host.rtx_write_image(b.encode(), w, h, rgb.ctypes.data) == 0
                out["write"][rp.write_name(w, h, ext)] = {
                    "input_sha256": rp.image_pin(rgb)["sha256"],
                    "ref_reads_ref": rp.image_pin(rp.ref_read(ref, a)),
                    "ref_reads_rtx": rp.image_pin(rp.ref_read(ref, b))}
        exe = os.path.join(tmp, "traceui_adapter_check")
        subprocess.run(tta.checker_command(exe), check=True)
        out["traceui"] = {"sources_sha256": rp.adapter_sources_sha(), "rows": tta.checker_rows(exe)}
    with open(rp.PINS_JSON, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {os.path.relpath(rp.PINS_JSON, ROOT)}: {len(out['tokens'])} token streams, "
          f"{len(out['images'])} images, {len(out['write'])} written files, {len(out['traceui']['rows'])} adapter rows")


if __name__ == "__main__":
    main()
