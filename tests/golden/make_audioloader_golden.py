"""Makes tests/golden/audioloader_cases.json.gz: the reference's own AudioLoader (stable_whisper/audio/__init__.py) driven
with the seeded cases of tests/test_audio_cpu.py::test_audioloader_matches_reference, every result in the JSON form of
``_canon`` (tensors as dtype, shape and the SHA-256 of their bytes).  Needs the reference checkout importable.

    python tests/golden/make_audioloader_golden.py
"""
import gzip
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as G  # noqa: E402
import test_audio_cpu as T  # noqa: E402

G.import_reference()
import stable_whisper.audio as RA  # noqa: E402

out = {}
for seed in range(60):
    mp = pytest.MonkeyPatch()
    try:
        kw, ops, stream, src_ref, _ = T._loader_case(seed, mp, RA)
        out[str(seed)] = T._canon(T._run_loader(RA.AudioLoader, src_ref, stream, kw, ops))
    finally:
        mp.undo()
with gzip.GzipFile(T.GOLDEN_LOADER, "wb", mtime=0) as f:
    f.write(json.dumps(out, separators=(",", ":")).encode())
print(f"{len(out)} cases -> {T.GOLDEN_LOADER} ({os.path.getsize(T.GOLDEN_LOADER)} bytes)")
