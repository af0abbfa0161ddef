"""TFRecord input source: framing, CRC-32C, Example wire format, dataset calls, resize_image.

Pinned by: RFC 3720 CRC-32C known answers; tests/golden/shapes_red_test_head.tfrec = the first three records,
verbatim, of a TensorFlow-written data file the reference ships (tools/gen_tfrecord_fixture.py) -- their embedded
masked checksums were computed by TensorFlow.  JPEG pixels are decoded by Pillow: agreement with TF's decoder is
unpinned (TensorFlow is not installed anywhere this runs).
"""
import glob
import io
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests/golden/shapes_red_test_head.tfrec")


def lt():
    from yolo_v3_tf2_amd.core import load_tfrecords
    return load_tfrecords


def test_crc32c_known_answers():
    m = lt()
    assert m.crc32c(b"") == 0
    assert m.crc32c(b"123456789") == 0xE3069283            # the standard check value
    assert m.crc32c(bytes(32)) == 0x8A9136AA                # RFC 3720 B.4
    assert m.crc32c(b"\xff" * 32) == 0x62A8AB43
    assert m.crc32c(bytes(range(32))) == 0x46DD794E
    assert m.crc32c(bytes(range(31, -1, -1))) == 0x113FDB5C
    # every tail length of the 8-byte sliced loop agrees with a bitwise loop
    data = np.random.default_rng(5).integers(0, 256, 67, dtype=np.uint8).tobytes()

    def slow(b):
        c = 0xFFFFFFFF
        for x in b:
            c ^= x
            for _ in range(8):
                c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
        return c ^ 0xFFFFFFFF
    for n in range(0, 67):
        assert m.crc32c(data[:n]) == slow(data[:n])


def test_reads_tensorflow_written_records():
    m = lt()
    recs = list(m.read_records(FIXTURE))          # both checksums of every record verified
    assert len(recs) == 3
    ex = m.parse_example(recs[0])
    assert sorted(ex) == ["image/encoded", "image/object/bbox/xmax", "image/object/bbox/xmin",
                          "image/object/bbox/ymax", "image/object/bbox/ymin", "image/object/class/text"]
    assert ex["image/object/class/text"] == [b"triangle", b"circle", b"circle"]
    assert ex["image/encoded"][0][:3] == b"\xff\xd8\xff"                 # a JPEG
    np.testing.assert_array_equal(ex["image/object/bbox/xmin"],
                                  np.array([0.7692308, 0.7956731, 0.5168269], np.float32))
    for r in recs:
        e = m.parse_example(r)
        n = len(e["image/object/class/text"])
        for k in ("xmin", "ymin", "xmax", "ymax"):
            v = e[f"image/object/bbox/{k}"]
            assert v.dtype == np.float32 and v.shape == (n,) and (v >= 0).all() and (v <= 1).all()
        assert (e["image/object/bbox/xmin"] < e["image/object/bbox/xmax"]).all()


def test_corruption_and_truncation_raise(tmp_path):
    m = lt()
    raw = bytearray(open(FIXTURE, "rb").read())
    bad = tmp_path / "bad.tfrec"
    raw[40] ^= 1                                   # payload bit flip
    bad.write_bytes(raw)
    with pytest.raises(ValueError, match="corrupted record data"):
        list(m.read_records(str(bad)))
    assert len(list(m.read_records(str(bad), check_crc=False))) == 3
    raw[40] ^= 1
    raw[2] ^= 1                                    # length field
    bad.write_bytes(raw)
    with pytest.raises(ValueError, match="corrupted record length"):
        list(m.read_records(str(bad)))
    raw[2] ^= 1
    bad.write_bytes(raw[:-7])
    with pytest.raises(ValueError, match="truncated"):
        list(m.read_records(str(bad)))


from tests.helpers import jpeg_bytes as _jpeg, make_tfrecord_dataset as make_dataset  # noqa: E402


def test_write_read_round_trip_and_dataset_calls(tmp_path):
    m = lt()
    rng = np.random.default_rng(11)
    truth = make_dataset(str(tmp_path), rng)
    names = tmp_path / "classes.names"
    names.write_text("circle\nsquare\n")
    exs = list(m.iter_examples(str(tmp_path)))
    assert len(exs) == 5
    for e, (jpg, lo, hi, lab) in zip(exs, truth):
        assert e["image/encoded"] == [jpg] and list(e["image/object/class/text"]) == lab
        np.testing.assert_array_equal(e["image/object/bbox/xmin"], lo[:, 0])
        np.testing.assert_array_equal(e["image/object/bbox/ymax"], hi[:, 1])
    ds = m.parse_tfrecords(str(tmp_path), image_size=32, max_bboxes=4, class_file=str(names))
    items = list(ds)
    assert len(items) == 5 and len(list(ds)) == 5          # re-iterable
    x, y = items[2]
    assert x.shape == (32, 32, 3) and x.dtype == np.float32 and 0 <= x.min() and x.max() <= 1
    assert y.shape == (4, 6)
    np.testing.assert_array_equal(y[:2, 4], [1, 1])         # objectness column, then zero padding
    np.testing.assert_array_equal(y[2:], 0)
    np.testing.assert_array_equal(y[:2, 5], [0, 1])         # class = line number in the names file
    assert items[4][1][0, 5] == 0 and items[4][1][1, 4] == 0 and items[3][1].sum() == 0   # 1 box; no boxes
    # reference call pattern: evaluate_yolov3.py:86-94 / inference.py:121-123
    batches = list(ds.batch(2).map(lambda img, yy: (img * 2, yy)))
    assert [b[0].shape[0] for b in batches] == [2, 2, 1]
    np.testing.assert_array_equal(batches[1][0][0], items[2][0] * 2)
    only_img = list(ds.batch(4, drop_remainder=True).map(lambda img, _: img))
    assert len(only_img) == 1 and only_img[0].shape == (4, 32, 32, 3)
    no_table = list(m.parse_tfrecords(str(tmp_path), 32, 4))
    assert no_table[2][1].shape == (4, 5)
    with pytest.raises(ValueError, match="exceed max_bboxes"):
        list(m.parse_tfrecords(str(tmp_path), 32, 1))
    # unknown label -> -1 (StaticHashTable default)
    e = m.parse_example(m.make_example({"image/encoded": truth[0][0], "image/object/class/text": [b"zebra"],
                                        "image/object/bbox/xmin": [0.1], "image/object/bbox/ymin": [0.1],
                                        "image/object/bbox/xmax": [0.2], "image/object/bbox/ymax": [0.2]}))
    assert m.example_boxes(e, m.load_class_table(str(names)))[0, 5] == -1


def test_unpacked_float_and_int64_lists_parse():
    m = lt()
    # FloatList written unpacked (one fixed32 field per value) and an Int64List, packed and with a negative value
    f_unpacked = b"".join(b"\x0d" + np.float32(v).tobytes() for v in (0.25, 0.5))
    feat_f = m._ld(2, f_unpacked)
    feat_i = m._ld(3, m._ld(1, bytes([5, 0xAC, 0x02]) + b"\xff" * 9 + b"\x01"))
    ex = m._ld(1, m._ld(1, m._ld(1, b"f") + m._ld(2, feat_f)) + m._ld(1, m._ld(1, b"i") + m._ld(2, feat_i)))
    out = m.parse_example(ex)
    np.testing.assert_array_equal(out["f"], np.array([0.25, 0.5], np.float32))
    np.testing.assert_array_equal(out["i"], np.array([5, 300, -1], np.int64))


def test_resize_image_keeps_aspect_and_centres():
    from yolo_v3_tf2_amd.core.utils import resize_bilinear, resize_image
    rng = np.random.default_rng(3)
    img = rng.random((50, 100, 3), dtype=np.float32)
    out = resize_image(img, 64, 64)                  # scale 0.64 -> 32 x 64, 16 rows of zeros above and below
    assert out.shape == (64, 64, 3)
    np.testing.assert_array_equal(out[:16], 0)
    np.testing.assert_array_equal(out[48:], 0)
    np.testing.assert_array_equal(out[16:48], resize_bilinear(img, 32, 64))
    tall = resize_image(rng.random((90, 30, 3), dtype=np.float32), 60, 60)     # -> 60 x 20, 20 columns each side
    np.testing.assert_array_equal(tall[:, :20], 0)
    np.testing.assert_array_equal(tall[:, 40:], 0)
    assert (tall[:, 20:40] > 0).all()
    sq = rng.random((2, 48, 48, 3), dtype=np.float32)                            # the inference.py:123 case: identity
    np.testing.assert_array_equal(resize_image(sq, 48, 48), sq)
    # round-half-even of the scaled size: 5 x 3 -> target 2 x 2: scale 0.4 -> (2.0, 1.2) -> 2 x 1
    assert (resize_image(np.ones((5, 3, 1), np.float32), 2, 2)[:, :, 0] == [[1, 0], [1, 0]]).all()


def test_every_reference_tfrecord_file_reads_clean(tmp_path):
    """Every record of every three_mixed_shapes TFRecord file the reference ships (tests/golden/
    shapes_three_mixed_tfrecords_blanked.tar.xz, made by tools/gen_tfrecord_fixture.py --bundle): TensorFlow's lengths, both
    checksums and Example bytes verbatim; only the JPEG bytes are zeroed, with four of them set so the data checksum holds."""
    import tarfile
    m = lt()
    with tarfile.open(os.path.join(ROOT, "tests/golden/shapes_three_mixed_tfrecords_blanked.tar.xz")) as tar:
        for member in tar.getmembers():
            assert member.isfile() and not member.name.startswith(("/", "..")) and ".." not in member.name.split("/")
            (tmp_path / member.name).parent.mkdir(parents=True, exist_ok=True)
            (tmp_path / member.name).write_bytes(tar.extractfile(member).read())
    files = sorted(glob.glob(str(tmp_path / "three_mixed_shapes/*/input/tfrecords/*/*.tfrec")))
    assert len(files) == 6
    total = 0
    for f in files:
        for rec in m.read_records(f):
            e = m.parse_example(rec)
            # (the "white" files carry image/object/class/label instead of .../text)
            labels = e.get("image/object/class/text", e.get("image/object/class/label"))
            assert len(e["image/encoded"]) == 1 and len(labels) == len(e["image/object/bbox/xmin"])
            total += 1
    assert total == 900


def test_evaluate_driver_host_pieces(tmp_path):
    """arrange_predict_output / prepare_dataset / calc_recal_precision of the evaluation driver (no GPU)."""
    from yolo_v3_tf2_amd import evaluate_yolov3 as ev
    rng = np.random.default_rng(2)
    B, N, M = 2, 30, 5
    bb = rng.random((B, N, 4)).astype(np.float32)
    cc = rng.integers(0, 3, (B, N)).astype(np.int64)
    ss = rng.random((B, N)).astype(np.float32)
    sel = np.stack([rng.permutation(N)[:M] for _ in range(B)]).astype(np.int32)
    nv = np.array([3, 0], np.int32)
    gt = np.concatenate([rng.random((B, 2, 4)), np.ones((B, 2, 1)), [[[1], [2]], [[0], [0]]]], axis=-1).astype(np.float32)
    pb, pc, gb, gc = ev.arrange_predict_output(bb, cc, ss, sel, nv, gt)
    assert [len(x) for x in pb] == [3, 0] and np.array_equal(pb[0], bb[0][sel[0][:3]]) and np.array_equal(pc[0], cc[0][sel[0][:3]])
    assert gb.shape == (2, 2, 4) and gc.dtype == np.int32 and gc.tolist() == [[1, 2], [0, 0]]
    r, p = ev.calc_recal_precision({"tp": np.array([2, 0]), "fp": np.array([2, 0]), "fn": np.array([0, 3])})
    assert np.allclose(r, [1, 0]) and np.allclose(p, [0.5, 0])
    # dataset: 4 records, each with exactly two boxes -> batches of 2 stack
    m = lt()
    payloads = []
    for i in range(4):
        payloads.append(m.make_example({"image/encoded": _jpeg(rng, 40, 60), "image/object/class/text": [b"b", b"a"],
                                        "image/object/bbox/xmin": [0.1, 0.2], "image/object/bbox/ymin": [0.1, 0.2],
                                        "image/object/bbox/xmax": [0.5, 0.6], "image/object/bbox/ymax": [0.5, 0.6]}))
    m.write_records(str(tmp_path / "x.tfrec"), payloads)
    (tmp_path / "c.names").write_text("a\nb\n")
    batches = list(ev.prepare_dataset(str(tmp_path), 2, 32, 10, str(tmp_path / "c.names")))
    assert len(batches) == 2 and batches[0][0].shape == (2, 32, 32, 3) and batches[0][1].shape == (2, 2, 6)
    assert batches[0][1][0, :, 5].tolist() == [1, 0]
