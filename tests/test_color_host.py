"""Colour files on the CPU: the chroma constants of the library and the CPU model the GPU tests compare against
(tests/color_model.py).  No compute calls are made here."""
from __future__ import annotations

import io

import numpy as np
import pytest

import color_model as cm
import scan_model as sm

QUALITIES = (1, 10, 50, 75, 90, 100)


def test_chroma_quant_tables_are_annex_k_and_its_scaling(jpegamd):
    k2 = np.array(cm.CHROMA_Q, np.uint8)
    assert np.array_equal(jpegamd.chroma_quant_table(50), k2)
    assert np.array_equal(jpegamd.chroma_quant_table(0), k2)
    for q in QUALITIES:
        assert np.array_equal(jpegamd.chroma_quant_table(q), cm.scaled_table(cm.CHROMA_Q, q)), q
        assert np.array_equal(jpegamd.quant_table(q), cm.scaled_table(cm.LUMA_Q, q)), q      # the rule is the luma table's
    assert jpegamd.chroma_quant_table(100).max() == 1 and jpegamd.chroma_quant_table(1).min() == 255


@pytest.mark.parametrize("q", QUALITIES)
def test_chroma_guard_band_holds_on_float32_emulation(jpegamd, oracle, q):
    """test_host.py::test_mfma_guard_band_holds_on_float32_emulation for the chroma table: the matrix pipe's two exact chains, the
    one add that joins them, the kernel's fma; an unflagged coefficient must equal the reference-order value quantised with the
    chroma table, and |z_fast - z_ref| stays below the table's delta."""
    f32, f64 = np.float32, np.float64
    zz = cm.ZIGZAG
    lut = jpegamd.cos_lut()
    K = np.zeros((64, 64))
    for k in range(64):
        u, v = divmod(k, 8)
        K[k] = np.outer(lut[:, u].astype(f64), lut[:, v].astype(f64)).reshape(64)
    hi = np.rint(K * 2048.0)
    lo = np.rint((K - hi / 2048.0) * 4194304.0) / 2048.0
    rng = np.random.default_rng(5 + q)
    blocks = [rng.integers(-128, 128, 64) for _ in range(120)] + [np.full(64, v) for v in (-128, 127, 3, -77)]
    blocks += [np.where(K[k] >= 0, 127, -128) for k in (1, 9, 27, 63)] + [rng.integers(-4, 5, 64) + 100 for _ in range(20)]
    P = np.array(blocks, dtype=np.int64)
    ref = oracle.dct_blocks(P.reshape(-1, 8, 8).astype(np.int8)).reshape(-1, 64)
    Y = (P + 128).astype(f64) * 2.0 ** -24
    c = jpegamd.chroma_mfma_consts(q)
    table = jpegamd.chroma_quant_table(q).astype(f32)
    chains = []
    for t in (lo, hi):
        prod = (t[None, :, :] * Y[:, None, :]).astype(f32)
        acc = np.zeros((len(P), 64), f32)
        for i in range(64):
            acc = (acc + prod[:, :, i]).astype(f32)
        assert np.array_equal(acc.astype(f64), (Y[:, None, :] * t[None, :, :]).sum(axis=2))      # exact
        chains.append(acc)
    acc = (chains[1] + chains[0]).astype(f32)
    acc[:, 0] = (acc[:, 0] - f32(c["dc_off"])).astype(f32)
    unflagged = 0
    for z in range(64):
        k = zz[z]
        zc = (acc[:, k].astype(f64) * f64(c["qmul"][z]) + f64(f32(c["qadd"][z]))).astype(f32)
        n = np.floor(zc).astype(np.int64)
        flagged = (zc - np.floor(zc)) <= f32(c["qthr"][z])
        want = np.array([int(np.float32(np.round(np.float32(r) / table[k]))) if abs(np.float32(r) / table[k]) % 1 != 0.5
                         else int(np.sign(r) * np.ceil(abs(np.float32(r) / table[k]))) for r in ref[:, k]], np.int64)
        assert np.array_equal(n[~flagged], want[~flagged]), (q, z)
        z_fast = acc[:, k].astype(f64) * f64(c["qmul"][z]) + f64(f32(c["zoff"][z]))
        assert np.abs(z_fast - ref[:, k].astype(f64) / f64(table[k])).max() <= c["delta"][k], (q, z)
        unflagged += int((~flagged).sum())
    assert unflagged > 0.9 * acc.size


def test_max_jfif_bytes_color_bounds(jpegamd):
    for w, h in ((1, 1), (7, 9), (8192, 8192)):
        nb = ((w + 7) // 8) * ((h + 7) // 8)
        c420 = jpegamd.max_jfif_bytes_color(w, h, jpegamd.SUBSAMPLE_420)
        c444 = jpegamd.max_jfif_bytes_color(w, h, jpegamd.SUBSAMPLE_444)
        assert c444 >= c420 > 2 * nb * 1723 // 8
        assert c444 >= 3 * 2 * (nb * 1723 // 8)
    assert jpegamd.max_jfif_bytes_color(8, 8, 0) == 0 and jpegamd.max_jfif_bytes_color(8, 8, 3) == 0
    assert jpegamd.max_jfif_bytes_color(0, 8, 1) == 0


def test_model_packer_matches_the_oracle_on_luma(oracle, jpegamd):
    """The model's Huffman packer, run with the luma tables, is the oracle's own entropy coder."""
    for (w, h, seed, kind) in ((53, 37, 3, 0), (40, 17, 4, 1), (64, 64, 2, 3)):
        st = oracle.stages(jpegamd.synth_bmp(w, h, seed, kind, 0))
        assert sm.pack_scan(oracle, st["zigzag"], False) == oracle.entropy(st["zigzag"])


def test_model_prefix_shares_the_grayscale_headers(oracle):
    gray = oracle.jfif_prefix(53, 37, 50)
    col = cm.color_prefix(53, 37, 0, cm.SUB_420)
    assert col[:20] == gray[:20]                                   # SOI + APP0
    dht_l = gray[gray.index(b"\xff\xc4"):gray.index(b"\xff\xda")]   # the two luma DHT segments
    assert dht_l in col
    assert col.endswith(cm.sos(1)) and col.count(b"\xff\xc4") == 4


@pytest.mark.parametrize("sub", (cm.SUB_420, cm.SUB_444))
def test_model_colour_file_decodes_with_pil(oracle, jpegamd, sub):
    from PIL import Image
    from jpegamd import quality as jq
    # (RGB, per-channel) floors, 1.5-2 dB under what this model measured at Q 50: photo-like 27.8 / 27.9 (Y), gradients 35.3 / 37.6 (Cb)
    floors = {0: (26.0, 26.0), 3: (33.0, 35.0)}
    for (w, h, seed, kind) in ((53, 37, 3, 0), (40, 17, 4, 3), (8, 8, 1, 0), (1, 1, 2, 0), (96, 64, 9, 1)):
        bmp = jpegamd.synth_bmp(w, h, seed, kind, 0)
        jf = cm.color_file(oracle, bmp, 0, sub)
        img = Image.open(io.BytesIO(jf))
        img.load()
        assert img.mode == "RGB" and img.size == (w, h)
        r = jq.analyze_color(bmp, jf)
        if kind != 1 and w * h >= 64:                              # (noise and single pixels: decodability only)
            assert r["psnr_rgb"] > floors[kind][0], (w, h, kind, r)
            assert min(r["psnr_y"], r["psnr_cb"], r["psnr_cr"]) > floors[kind][1], (w, h, kind, r)


def test_model_chroma_planes_follow_the_spec():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]], [[255, 255, 255], [0, 0, 0], [10, 20, 30]]], np.uint8)
    cb, cr = cm.chroma_planes(rgb, cm.SUB_444)
    r, g, b = 10, 20, 30
    assert cb[1, 2] == (32768 - 43 * r - 85 * g + 128 * b) >> 8 and cr[1, 2] == (32768 + 128 * r - 107 * g - 21 * b) >> 8
    assert cb[1, 0] == 128 and cr[1, 0] == 128 and cb[1, 1] == 128
    c2, _ = cm.chroma_planes(rgb, cm.SUB_420)
    assert c2.shape == (1, 2)
    assert c2[0, 1] == (int(cb[0, 2]) * 2 + int(cb[1, 2]) * 2 + 2) >> 2      # the odd last column replicated


def test_gray_order_and_colour_entries_are_declared(jpegamd):
    assert jpegamd.ORDER_GRAY == 2 and (jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_420) == (1, 2)
    for name in ("jpegamd_encode_color_async", "jpegamd_encode_bmp_memory_color", "jpegamd_max_jfif_bytes_color"):
        assert name in jpegamd.EXPORTED and hasattr(jpegamd.lib, name)


# ---- the fixture builders of tests/test_gpu_color_edges.py (tests/color_fixtures.py) ---------------------------------------
def test_rgb_for_plane_meets_the_target_plane_exactly():
    import color_fixtures as cf
    rng = np.random.default_rng(12)
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    for target in (every, rng.integers(0, 256, (9, 13), np.uint8), np.zeros((3, 5), np.uint8), np.full((2, 7), 255, np.uint8)):
        base = rng.integers(0, 256, target.shape, np.uint8)
        for which, idx in (("cb", 0), ("cr", 1)):
            for sub in (cm.SUB_444, cm.SUB_420):
                for b in (None, base):
                    rgb = cf.rgb_for_plane(target, which, sub, base=b)
                    assert np.array_equal(cm.chroma_planes(rgb, sub)[idx], target), (which, sub, target.shape)
            # odd picture sizes at 4:2:0: the last column / row replicated, the plane unchanged
            h, w = 2 * target.shape[0] - 1, 2 * target.shape[1] - 1
            rgb = cf.rgb_for_plane(target, which, cm.SUB_420, shape=(h, w))
            assert rgb.shape == (h, w, 3) and np.array_equal(cm.chroma_planes(rgb, cm.SUB_420)[idx], target)


def test_chroma_symbol_fixture_covers_every_symbol_class(oracle):
    """The chroma scan of the symbol fixture holds every DC size 0..11, every AC size 1..10, every run 0..15, ZRLs, EOBs and a block
    whose zigzag 63 is non-zero -- counted from the model's own symbol list, so the fixture cannot quietly lose any of them."""
    import color_fixtures as cf
    plane = cf.symbol_plane(oracle)
    cov = cf.chroma_symbol_coverage(oracle, plane)
    assert cov["dc_sizes"] == set(range(12))
    assert cov["sizes"] == set(range(1, 11))
    assert cov["runs"] == set(range(16))
    assert cov["zrl"] > 0 and cov["eob"] > 0 and cov["no_eob"] > 0
    # of the 162 K.6 codes (EOB, ZRL, 16 runs x 10 sizes) a baseline block cannot make every one (at most 63 - run
    # positions, and high frequencies cap the amplitude); measured 132 when the fixture was written
    reached = len(cov["codes"]) + 2
    print(f"chroma symbol fixture: {reached} of 162 K.6 codes, {plane.shape[1] // 8} x {plane.shape[0] // 8} blocks")
    assert reached >= 130
    # the fixture's blocks through the RGB pictures the GPU test sends
    for which, idx in (("cb", 0), ("cr", 1)):
        for sub in (cm.SUB_444, cm.SUB_420):
            assert np.array_equal(cm.chroma_planes(cf.rgb_for_plane(plane, which, sub), sub)[idx], plane)


def test_chroma_tie_fixture_sits_on_rounding_ties(jpegamd, oracle):
    """At the tie quality, many coefficients of the tie plane, exact-order value over the chroma step, lie within the guard band
    (the chroma constants' delta) of a half: the kernel cannot settle them on the fast path and must take the exact-order fallback."""
    import color_fixtures as cf
    plane = cf.tie_plane()
    h, w = plane.shape
    blocks = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 8, 8)
    f = oracle.dct_blocks((blocks.astype(np.int16) - 128).astype(np.int8)).reshape(-1, 64).astype(np.float64)
    z = f / cm.scaled_table(cm.CHROMA_Q, cf.TIE_QUALITY).astype(np.float64)[None, :]
    near = np.abs(np.abs(z) % 1 - 0.5) <= jpegamd.chroma_mfma_consts(cf.TIE_QUALITY)["delta"][None, :]
    assert near.sum() >= 100


def test_extreme_plane_is_the_grayscale_block_set(jpegamd):
    import color_fixtures as cf
    blocks = cf.extreme_blocks(jpegamd.cos_lut())
    assert len(blocks) == 64 * 4 + 4 + 6 + 58
    p = cf.extreme_plane(jpegamd.cos_lut())
    assert p.shape == (8 * ((len(blocks) + 39) // 40), 320) and set(np.unique(p)) <= {0, 1, 127, 128, 255}
