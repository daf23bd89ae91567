#!/usr/bin/env python3
"""Record the reference parser's answers under tests/golden/reference_settings/.

tests/test_reference_pins.py holds host/settings.cpp to the reference's own settings parser (settings.cu + log.cu,
compiled host-only by `make -C oracle ref` where the reference's sources are).  Its answers to the test's requests -
on the shipped settings.txt (stored beside them, byte for byte) and on the grammar cases - are stored here so that the
test runs where the reference is absent; where the binary exists the test asks it again.  Run from the repo root after
`make -C oracle ref`:  python tests/golden/make_reference_settings.py
"""
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_reference_pins as t  # noqa: E402


def record(name, path, requests, tmp):
    out = os.path.join(tmp, name + ".out")
    t._dump(t.REF_DUMP, path, requests, out)
    shutil.copyfile(out, os.path.join(t.GOLD, name + ".ref.txt"))


def main():
    if not os.path.exists(t.REF_DUMP):
        raise SystemExit(f"{t.REF_DUMP} is missing: build it with `make -C oracle ref` where the reference's sources are")
    with tempfile.TemporaryDirectory() as tmp:
        record("shipped", t.SETTINGS, t.shipped_requests()[1], tmp)
        for name, text in t.GRAMMAR_CASES.items():
            path = os.path.join(tmp, name + ".txt")
            with open(path, "wb") as f:
                f.write(text.encode())
            record(name, path, t.case_requests(text), tmp)
    print("recorded", sorted(os.listdir(t.GOLD)))


if __name__ == "__main__":
    main()
