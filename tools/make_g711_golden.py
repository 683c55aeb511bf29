"""Writes tests/golden/g711.npz: the two 65 536-entry G.711 encode tables (inputs −32768 … 32767 in order) and the two 256-entry decode
tables, produced with CPython's audioop (width 2) — the Sun g711.c definition that include/piper_hip.h "G.711 output" states. The tests
compare the numpy reference, the host functions and the device against these, so a machine that runs them needs no audioop.

    python tools/make_g711_golden.py            (audioop: CPython up to 3.12)
"""
import audioop
import hashlib
import os

import numpy as np

HASHES = {"mulaw": "81d633c9e6972a18c74a58720b96cb8ca0bdd096d4060b646dd708c3b846019a",
          "alaw": "38488f6fd710f4686360edc4d38639f96c491595ef93f8eb8d62d5e07ca6ce7b"}


def main():
    pcm = np.arange(-32768, 32768, dtype=np.int32).astype("<i2").tobytes()
    codes = bytes(range(256))
    out = {"mulaw_encode": np.frombuffer(audioop.lin2ulaw(pcm, 2), np.uint8), "alaw_encode": np.frombuffer(audioop.lin2alaw(pcm, 2), np.uint8),
           "mulaw_decode": np.frombuffer(audioop.ulaw2lin(codes, 2), "<i2").astype(np.int16),
           "alaw_decode": np.frombuffer(audioop.alaw2lin(codes, 2), "<i2").astype(np.int16)}
    for law, want in HASHES.items():
        got = hashlib.sha256(out[law + "_encode"].tobytes()).hexdigest()
        assert got == want, (law, got)
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g711.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
