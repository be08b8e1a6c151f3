"""Regenerates tests/golden/ref_reader_chunks.json (committed): what the
reference's own InputFileHandler/FASTQFileReader hand out as chunks for the
odd inputs of tests/test_oracle.py::test_reader_matches_reference_reader, at
every chunk size that test uses. Recorded output of oracle/_ref/ref_reader
(the reference's reader compiled unmodified, oracle/ref/Makefile), so the test
also runs where that program cannot be built. Per case: the input text and,
per chunk size, the list of [chunk bytes (latin-1), line length, n]: the chunk
is the bytes with their last byte repeated n more times (the reference pads a
file without a final newline up to the chunk size with the last quality byte,
a megabyte of it at the largest size).

Usage: python tests/golden/make_ref_reader_chunks.py   (needs oracle/_ref)
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
import oracle  # noqa: E402
import test_oracle  # noqa: E402


def entry(b, ll):
    s = b.decode("latin-1")
    head = s.rstrip(s[-1:]) + s[-1:]
    return [head, ll, len(s) - len(head)]


def main():
    lines = []
    for name, text in sorted(test_oracle._weird_cases().items()):
        with tempfile.TemporaryDirectory() as d:
            with open(os.path.join(d, "a.fq"), "w", newline="") as f:
                f.write(text)
            chunks = {str(c): [entry(b, ll) for b, ll in oracle.ref_chunks(d, c)]
                      for c in test_oracle.READER_CHUNKS}
        lines.append(f"{json.dumps(name)}: {json.dumps({'input': text, 'chunks': chunks}, separators=(',', ':'))}")
    with open(os.path.join(HERE, "ref_reader_chunks.json"), "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")


if __name__ == "__main__":
    main()
