"""The threshold fixtures (tests/threshold_fixtures.py) through the kernels, byte for byte against the oracle.

Every picture of tests/golden/thresholds.json sits on an edge of k_tile_encode, k_segment_merge or k_stitch that
tests/test_thresholds_host.py has proven on the CPU; here each goes through jpegamd_encode_async and jpegamd_encode_batch_async (2
pictures: segments of 8 tiles; 4 and 5: of 16) under both pipelines, as one-byte luma and as the BGR BMP of the same values,
bottom-up and top-down.  One context per geometry is reused across fixtures, so the scratch a dense picture left meets a sparse
one.  Nothing here reads the reference tree."""
from __future__ import annotations

import ctypes
from collections import defaultdict

import numpy as np
import pytest

import color_fixtures as cf
import color_model as cm
import path_model as pm
import scan_model as sm
import threshold_fixtures as tf
from gpu_support import dev     # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def luma():
    """geometry -> [(spec, plane)]: the fixtures of one geometry, whatever their quality, share a context; a flat plane joins each
    geometry as a batch neighbour, so that a lone dense fixture still sits next to a sparse picture"""
    groups = defaultdict(list)
    for s in tf.fixtures():
        if s["plane"] == "luma":
            groups[(s["w"], s["h"])].append((s, tf.plane_of(s)))
    for (w, h), group in groups.items():
        group.append((dict(name="flat neighbour", quality=group[0][0]["quality"]), np.full((h, w), 128, np.uint8)))
    return groups


@pytest.fixture(scope="module")
def want_of(oracle):
    """(fixture name, quality) -> the oracle's file of that plane at that quality"""
    cache = {}

    def want(name, y, q):
        key = (name, y.shape, q)                                           # (the flat neighbours of all geometries share a name)
        if key not in cache:
            cache[key] = oracle.encode_bmp(tf.gray_bmp(y), q)
        return cache[key]
    return want


def _run(jpegamd, enc, dev, planes, w, h, q, gray, top_down=True, cap=None):
    """planes: uint8 [h, w] pictures of one geometry -> (files, Stats, output buffers); one picture goes through the plain entry"""
    ups, imgs = [], []
    for y in planes:
        if gray:
            px = torch.from_numpy(np.ascontiguousarray(y if top_down else y[::-1])).to(dev)
            stride, order = w, jpegamd.ORDER_GRAY
        else:
            bmp = tf.gray_bmp(y, top_down)
            img, off = jpegamd.parse_bmp(bmp)
            px = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * img.height]), dtype=torch.uint8).to(dev)
            stride, order = img.row_stride, jpegamd.ORDER_BGR
        ups.append(px)
        imgs.append(jpegamd.Encoder.image(px.data_ptr(), w, h, stride, not top_down, order, q))
    cap = cap if cap is not None else jpegamd.max_jfif_bytes(w, h)
    outs = [torch.zeros(cap + 64, dtype=torch.uint8, device=dev) for _ in planes]
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in planes]
    stream = torch.cuda.current_stream().cuda_stream
    if len(planes) == 1:
        enc.encode_async(imgs[0], outs[0].data_ptr(), cap, sizes[0].data_ptr(), True, stream)
    else:
        enc.encode_batch_async(imgs, [o.data_ptr() for o in outs], cap, [s.data_ptr() for s in sizes], True, stream)
    st = enc.finish()
    return [bytes(o[:int(n.item())].cpu().numpy()) for o, n in zip(outs, sizes)], st, outs


def _first_diff(a: bytes, b: bytes):
    k = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return dict(first_differing_byte=k, lengths=(len(a), len(b)))


@pytest.mark.parametrize("pipeline", ["PAIR", "STITCH"])
def test_every_luma_fixture_alone_and_in_batches(jpegamd, dev, luma, want_of, pipeline):
    """A batch takes one quality for all its pictures: the neighbours -- the other fixtures of the geometry, cyclically -- are coded at
    the fixture's own."""
    for (w, h), group in luma.items():
        enc = jpegamd.Encoder(w, min(5 * h, 65528))
        enc.set_pipeline(getattr(jpegamd, "PIPELINE_" + pipeline))
        n = len(group)
        for i, (s, y) in enumerate(group[:-1]):
            q = s["quality"]
            want = want_of(s["name"], y, q)
            for gray, top_down in ((True, True), (False, False), (False, True), (True, False)):
                got = _run(jpegamd, enc, dev, [y], w, h, q, gray, top_down)[0][0]
                assert got == want, (s["name"], pipeline, "gray" if gray else "bgr", "top-down" if top_down else "bottom-up", _first_diff(got, want))
            for count in [c for c in (2, 4, 5) if c * h <= 65528]:
                batch = [group[i], group[-1]] + [group[(i + k) % n] for k in range(1, count - 1)]      # the flat picture comes second
                got = _run(jpegamd, enc, dev, [b[1] for b in batch], w, h, q, gray=bool(i % 2), top_down=True)[0]
                for g, b in zip(got, batch):
                    wb = want_of(b[0]["name"], b[1], q)
                    assert g == wb, (s["name"], pipeline, "batch of", count, b[0]["name"], _first_diff(g, wb))


STAT_FIXTURES = {"zrl_tail", "zrl_pair", "zrl_fell", "carry", "writeout1", "words121", "seg8_over", "seg8_w1", "seg16_over", "stale", "ladder",
                 "dense_q100", "long_tile"}


@pytest.mark.parametrize("pipeline", ["PAIR", "STITCH"])
def test_statistics_of_the_zrl_and_write_out_fixtures(jpegamd, oracle, dev, luma, want_of, pipeline):
    """entropy_bits and stuffed_bytes of the encoder's record against the oracle's symbols and scan, on the fixtures with ZRLs in each
    pass kind and with write-outs."""
    seen = set()
    for (w, h), group in luma.items():
        for s, y in group[:-1]:
            if s["name"] not in STAT_FIXTURES:
                continue
            seen.add(s["name"])
            q = s["quality"]
            want = want_of(s["name"], y, q)
            enc = jpegamd.Encoder(w, h)
            enc.set_pipeline(getattr(jpegamd, "PIPELINE_" + pipeline))
            got, st, _ = _run(jpegamd, enc, dev, [y], w, h, q, True)
            zz = oracle.stages(tf.gray_bmp(y), q)["zigzag"]
            sym, _, alen, is_dc, _ = sm.symbols(oracle, zz)
            bits = int((alen + np.where(is_dc, pm.LUMA.dc_len[sym & 15], pm.LUMA.ac_len[sym])).sum())
            assert got[0] == want
            assert st.entropy_bits == bits and (bits + 7) // 8 == len(pm.unstuff(want[328:-2])), s["name"]
            assert st.stuffed_bytes == want[328:-2].count(b"\xff\x00"), s["name"]
            assert st.jfif_bytes == len(want)
    assert seen == STAT_FIXTURES & {s["name"] for s in tf.fixtures()} and {"zrl_tail", "zrl_pair", "zrl_fell", "carry", "writeout1"} <= seen


def test_symbol_count_of_the_zrl_and_write_out_fixtures(jpegamd, oracle, dev, luma, want_of):
    """convertToJpeg's rle_count -- the tiles' t_all + nzrl, which k_tile_encode adds up separately in its tail, pair and quad passes --
    against the oracle's symbol list, where ZRLs sit in each pass kind and where the window is written out."""
    lib = jpegamd.lib
    assert lib.JpegCompression_Init() == 0
    seen = set()
    for (w, h), group in luma.items():
        for s, y in group[:-1]:
            if s["name"] not in STAT_FIXTURES:
                continue
            seen.add(s["name"])
            q = s["quality"]
            bmp = tf.gray_bmp(y)
            want = want_of(s["name"], y, q)
            img, off = jpegamd.parse_bmp(bmp)
            px = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * img.height]), dtype=torch.uint8).to(dev)
            cap = jpegamd.max_jfif_bytes(w, h)
            huff = torch.zeros(cap, dtype=torch.uint8, device=dev)
            y8, dct, quant, zz0 = (ctypes.c_int8 * 64)(), (ctypes.c_float * 64)(), (ctypes.c_int16 * 64)(), (ctypes.c_int16 * 64)()
            dto = jpegamd.DTO(width=w, height=h, r_phy_ptr=px.data_ptr(), huff_phy_ptr=huff.data_ptr(), huff_size=cap,
                              y_phy_ptr=ctypes.addressof(y8), dct_phy_ptr=ctypes.addressof(dct), quant_phy_ptr=ctypes.addressof(quant),
                              zigzag_phy_ptr=ctypes.addressof(zz0), row_stride=img.row_stride, bottom_up=img.bottom_up,
                              channel_order=jpegamd.ORDER_BGR, quality=q)
            assert lib.convertToJpeg(ctypes.byref(dto)) == 0, s["name"]
            zz = oracle.stages(bmp, q)["zigzag"]
            assert bytes(huff[:dto.huff_size].cpu().numpy()) == want[328:-2], s["name"]
            assert dto.rle_count == len(oracle.rle_symbols(zz)), (s["name"], dto.rle_count, len(oracle.rle_symbols(zz)))
    assert {"zrl_tail", "zrl_pair", "zrl_fell", "carry", "writeout1"} <= seen


@pytest.mark.parametrize("pipeline,name", [("PAIR", "seg8_over"), ("STITCH", "seg16_over")])
def test_exact_capacity_and_one_byte_short_on_a_slow_path_fixture(jpegamd, dev, luma, want_of, pipeline, name):
    """seg8_over: the slow merge of 8-tile segments; seg16_over: two stitch parts (k_stitch works on 16-tile segments)."""
    (s, y), = [f for g in luma.values() for f in g if f[0]["name"] == name]
    rep = tf.report_of(s, False)[0]
    assert not tf.S8(rep)["merge_fast"] if pipeline == "PAIR" else tf.S16(rep)["stitch_parts"] >= 2
    w, h, q = s["w"], s["h"], s["quality"]
    want = want_of(name, y, q)
    enc = jpegamd.Encoder(w, h)
    enc.set_pipeline(getattr(jpegamd, "PIPELINE_" + pipeline))
    got, _, outs = _run(jpegamd, enc, dev, [y], w, h, q, True, cap=len(want))
    assert got[0] == want
    assert bytes(outs[0][len(want):].cpu().numpy()) == bytes(64)                          # nothing written past the capacity
    cap = len(want) - 1
    px = torch.from_numpy(y).to(dev)
    out = torch.zeros(len(want) + 64, dtype=torch.uint8, device=dev)
    size = torch.zeros(1, dtype=torch.int64, device=dev)
    enc.encode_async(jpegamd.Encoder.image(px.data_ptr(), w, h, w, False, jpegamd.ORDER_GRAY, q), out.data_ptr(), cap, size.data_ptr(), True,
                     torch.cuda.current_stream().cuda_stream)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8 and int(size.item()) == len(want)                       # grayscale reports the would-be size
    assert bytes(out[cap:].cpu().numpy()) == bytes(len(want) + 64 - cap)                # nothing written past the capacity


@pytest.mark.parametrize("pipeline", ["PAIR", "STITCH"])
def test_chroma_fixtures_as_the_cb_plane_of_444_colour_pictures(jpegamd, oracle, dev, pipeline):
    """Alone (8-tile segments under the pair, 16-tile under k_stitch) and as a batch of four (eight chroma planes per launch: 16-tile
    segments under the pair as well), neighbours of the same geometry and quality cyclically."""
    groups = defaultdict(list)
    for s in tf.fixtures():
        if s["plane"] == "cb":
            rgb = cf.rgb_for_plane(tf.plane_of(s), "cb", cm.SUB_444)
            assert (cm.chroma_planes(rgb, cm.SUB_444)[0] == tf.plane_of(s)).all(), s["name"]
            groups[(s["w"], s["h"], s["quality"])].append((s, rgb, cm.color_file(oracle, cm.write_bmp(rgb), s["quality"], cm.SUB_444)))
    assert groups
    stream = torch.cuda.current_stream().cuda_stream
    for (w, h, q), group in groups.items():
        enc = jpegamd.Encoder(w, 4 * h)
        enc.set_pipeline(getattr(jpegamd, "PIPELINE_" + pipeline))
        cap = jpegamd.max_jfif_bytes_color(w, h, jpegamd.SUBSAMPLE_444)
        n = len(group)
        for i in range(n):
            for count in (1, 4):
                batch = [group[(i + k) % n] for k in range(count)]
                ups = [torch.from_numpy(np.ascontiguousarray(b[1])).to(dev) for b in batch]
                imgs = [jpegamd.Encoder.image(u.data_ptr(), w, h, 3 * w, False, jpegamd.ORDER_RGB, q) for u in ups]
                outs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in batch]
                sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in batch]
                if count == 1:
                    enc.encode_color_async(imgs[0], jpegamd.SUBSAMPLE_444, outs[0].data_ptr(), cap, sizes[0].data_ptr(), stream)
                else:
                    enc.encode_color_batch_async(imgs, jpegamd.SUBSAMPLE_444, [o.data_ptr() for o in outs], cap, [z.data_ptr() for z in sizes], stream)
                enc.finish()
                for o, z, b in zip(outs, sizes, batch):
                    got = bytes(o[:int(z.item())].cpu().numpy())
                    assert got == b[2], (group[i][0]["name"], pipeline, "batch of", count, b[0]["name"], _first_diff(got, b[2]))
