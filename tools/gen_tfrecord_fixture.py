#!/usr/bin/env python3
"""Cut the first records of one of the reference's TFRecord DATA files into a small test fixture.

The reference ships TensorFlow-written datasets (datasets/shapes/three_mixed_shapes/*/input/tfrecords/*/*.tfrec).
The bytes of a record -- framing, checksums, Example proto, JPEG -- are data written by TensorFlow itself, so the
first N records verbatim pin the reader in yolo-v3-tf2_amd/core/load_tfrecords.py (framing, CRC-32C masking, proto
wire format) against a genuine TF-written stream.  Output: tests/golden/shapes_red_test_head.tfrec.

Usage (in the build container, where /root/reference exists): python tools/gen_tfrecord_fixture.py [--records 3]

--bundle OUT --reference DIR: every record of every three_mixed_shapes TFRecord file of the reference tree DIR in one xz
tar (paths below datasets/shapes/, fixed member metadata so the bundle is reproducible):
tests/golden/shapes_three_mixed_tfrecords_blanked.tar.xz.  Each record keeps its length, both of TensorFlow's checksums and
every byte of its Example except the JPEG's: those become zeros (same length, so the proto is unchanged), and the last
four are chosen so that the data checksum TensorFlow wrote still matches.  The reader meets the TF-written framing,
checksums and Example of all 900 records; only the pixels are gone (they are most of the 6 MB).
"""
import argparse
import glob
import io
import os
import struct
import tarfile

SRC = "/root/reference/datasets/shapes/three_mixed_shapes/red/input/tfrecords/test/file_00_100.tfrec"


# CRC-32C (Castagnoli, reflected), written out here independently of the reader under test
_T = []
for _n in range(256):
    _c = _n
    for _ in range(8):
        _c = (_c >> 1) ^ (0x82F63B78 if _c & 1 else 0)
    _T.append(_c)
_TOP = {t >> 24: n for n, t in enumerate(_T)}       # the top byte of every table entry is distinct


def _advance(state, data):
    for x in data:
        state = (state >> 8) ^ _T[(state ^ x) & 0xFF]
    return state


def _retreat(state, data):
    """The register before `data`, given the register after it."""
    for x in reversed(data):
        n = _TOP[state >> 24]
        state = (((state ^ _T[n]) << 8) & 0xFFFFFFFF) | ((n ^ x) & 0xFF)
    return state


def _masked(data):
    c = _advance(0xFFFFFFFF, data) ^ 0xFFFFFFFF
    return ((((c >> 15) | (c << 17)) & 0xFFFFFFFF) + 0xA282EAD8) & 0xFFFFFFFF


def _varint(n):
    out = bytearray()
    while True:
        out.append((n & 0x7F) | (0x80 if n > 0x7F else 0))
        n >>= 7
        if not n:
            return bytes(out)


def blank_image(payload):
    """payload with the JPEG's bytes zeroed, the last four forged so that the CRC-32C of the whole payload is unchanged."""
    start, end = payload.index(b"\xff\xd8\xff"), payload.rindex(b"\xff\xd9") + 2
    assert payload[:start].endswith(_varint(end - start)), "the JPEG is not one whole bytes value"
    head, tail = payload[:start], payload[end:]
    want = _retreat(_advance(0xFFFFFFFF, payload), tail)        # register needed where the JPEG ends
    s = _advance(0xFFFFFFFF, head + bytes(end - start - 4))
    idx, t = [], want
    for _ in range(4):                                         # table indices of the four forged bytes, last first
        n = _TOP[t >> 24]
        idx.append(n)
        t = ((t ^ _T[n]) << 8) & 0xFFFFFFFF
    forged = bytearray()
    for n in reversed(idx):
        forged.append((s ^ n) & 0xFF)
        s = (s >> 8) ^ _T[n]
    assert s == want
    out = head + bytes(end - start - 4) + bytes(forged) + tail
    assert len(out) == len(payload) and _masked(out) == _masked(payload)
    return out


def bundle(reference, out):
    base = os.path.join(reference, "datasets", "shapes")
    files = sorted(glob.glob(os.path.join(base, "three_mixed_shapes", "*", "input", "tfrecords", "*", "*.tfrec")))
    with tarfile.open(out, "w:xz", preset=9) as tar:
        for path in files:
            blanked = io.BytesIO()
            with open(path, "rb") as f:
                while True:
                    head = f.read(12)
                    if not head:
                        break
                    (n,) = struct.unpack("<Q", head[:8])
                    payload, crc = f.read(n), f.read(4)
                    assert struct.unpack("<I", head[8:])[0] == _masked(head[:8]) and struct.unpack("<I", crc)[0] == _masked(payload)
                    blanked.write(head + blank_image(payload) + crc)     # TensorFlow's header and checksums, verbatim
            data = blanked.getvalue()
            info = tarfile.TarInfo(os.path.relpath(path, base))
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=3)
    ap.add_argument("--out", default="tests/golden/shapes_red_test_head.tfrec")
    ap.add_argument("--bundle", metavar="OUT", help="write the xz tar of every three_mixed_shapes file, images blanked, instead")
    ap.add_argument("--reference", metavar="DIR", help="root of the reference tree (with --bundle)")
    a = ap.parse_args()
    if a.bundle:
        print(f"{len(bundle(a.reference, a.bundle))} files -> {a.bundle}")
        return
    with open(SRC, "rb") as f, open(a.out, "wb") as o:
        for _ in range(a.records):
            head = f.read(12)
            (n,) = struct.unpack("<Q", head[:8])
            o.write(head + f.read(n + 4))


if __name__ == "__main__":
    main()
