"""Per-picture optimised Huffman tables in the one-scan colour files on the GPU (jpegamd_encoder_set_huffman): every
device file is compared byte for byte with the CPU model (tests/huffman_model.py).  tests/test_huffman_host.py proves on the CPU that
the pictures of tests/huffman_fixtures.py sit on the edges the cases claim.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import huffman_fixtures as hf
import huffman_model as hm
import interleaved_model as im
import mjpeg_support as ms
from gpu_support import dev  # noqa: F401
from huffman_fixtures import S420, S422, S444, SUBS

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_HUFF_CAPACITY = -8


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    """A context in OPTIMIZED for the whole module (the hygiene tests make their own)."""
    e = jpegamd.Encoder(1408, gs.rows_for(32, 16))
    e.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    yield e
    e.close()


def rgb_files(jpegamd, enc, rgbs, dev, sub, ri, q, cap=None):
    return gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "rgb", ri, q, cap=cap))


def check_rgb(jpegamd, oracle, enc, dev, rgbs, sub, ri, q):
    models = [hf.model(oracle, r, q, sub, ri) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, sub, ri, q)
    for f, m in zip(files, models):
        assert f[:m.prefix_len] == m.file[:m.prefix_len], (sub, ri)
        assert f == m.file, (sub, ri)
    assert st.entropy_bits == sum(m.scan_bits for m in models) and st.stuffed_bytes == sum(m.stuffed for m in models), (sub, ri)
    return models, files


def check_planes(jpegamd, oracle, enc, dev, planes, sub, ri, q):
    m = hf.planes_model(oracle, planes, q, sub, ri)
    (f,), st = ms.ycc_files(jpegamd, enc, ms.FULL8, [planes], dev, sub, ms.PLANES, ri, q)
    assert f == m.file
    assert st.entropy_bits == m.scan_bits and st.stuffed_bytes == m.stuffed
    return m


# ---- 1. content x geometry x interval -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h,kind,q", hf.CONTENT)
def test_content_geometry_and_interval(jpegamd, oracle, dev, enc, w, h, kind, q, sub):
    rgb = hf.content_rgb(w, h, kind)
    for ri in hf.INTERVALS:
        check_rgb(jpegamd, oracle, enc, dev, [rgb], sub, hf.interval(ri, w, sub), q)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("ri", (0, 5))
def test_batch_of_three_has_three_tables_and_prefix_lengths(jpegamd, oracle, dev, enc, sub, ri):
    rgbs = hf.batch_of_three()
    models, files = check_rgb(jpegamd, oracle, enc, dev, rgbs, sub, ri, 75)
    assert len({m.prefix_len for m in models}) == 3 and len({repr(m.tables) for m in models}) == 3


# ---- 2. the mode rides on every entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ri", (0, 3))
def test_limited_nv12_rgba_and_planar_sources(jpegamd, oracle, dev, enc, ri):
    stored = ms.stored_planes(ms.LIMITED8, 72, 40, S420, 41)
    m = hf.planes_model(oracle, ms.mapped_planes(ms.LIMITED8, stored, S420), 50, S420, ri)
    (f,), st = ms.ycc_files(jpegamd, enc, ms.LIMITED8, [stored], dev, S420, ms.CBCR, ri, 50)
    assert f == m.file and st.entropy_bits == m.scan_bits
    rgb = hf.synth_rgb(72, 40, 64)
    for sub in (S444, S422):
        want = hf.model(oracle, rgb, 50, sub, ri).file
        (f,), _ = gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, [rgb], dev, sub, "rgba", ri, 50))
        assert f == want
        (f,), _ = gs.finish_files(enc, ms.PlanarCall(jpegamd, enc, [rgb], dev, sub, ri, 50))
        assert f == want
        (f,), _ = gs.finish_files(enc, ms.OldRgbCall(jpegamd, enc, [rgb], dev, sub, ri, 50))
        assert f == want
    planes = ms.derived_planes(rgb, S420)
    (f,), _ = gs.finish_files(enc, ms.OldYccCall(jpegamd, enc, [planes], dev, S420, ms.PLANES, ri, 50))
    assert f == hf.planes_model(oracle, planes, 50, S420, ri).file


# ---- 3. single-symbol tables, short segments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,sub", hf.FLAT)
def test_flat_pictures_code_every_symbol_with_one_bit(jpegamd, oracle, dev, enc, w, h, sub):
    rgb = hf.flat(w, h)
    for ri in hf.FLAT_INTERVALS:
        (m,), _ = check_rgb(jpegamd, oracle, enc, dev, [rgb], sub, ri, 50)
        assert [len(t[1]) for t in m.tables] == [1, 1, 1, 1]


@pytest.mark.parametrize("ri", (0, 86))
def test_short_tail_that_borrows_bits_of_the_segment_in_front(jpegamd, oracle, dev, enc, ri):
    m = check_planes(jpegamd, oracle, enc, dev, hf.short_tail_planes(hf.BORROWED, ri), S444, ri, hf.BORROWED["quality"])
    assert m.borrowed_tails > 0


@pytest.mark.parametrize("ri", (0, 86))
def test_short_segment_that_completes_an_ff_byte(jpegamd, oracle, dev, enc, ri):
    m = check_planes(jpegamd, oracle, enc, dev, hf.short_tail_planes(hf.AGAINST_FF, ri), S444, ri, hf.AGAINST_FF["quality"])
    assert m.short_against_ff > 0 and m.stuffed > 0


# ---- 4. the length limit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,seed,q", hf.LONG_CODES)
def test_lengths_beyond_16_are_limited(jpegamd, oracle, dev, w, h, kind, seed, q):
    rgb = hf.synth_rgb(w, h, seed, kind)
    m = hf.model(oracle, rgb, q, S420, 0)
    assert max(t[2] for t in m.tables) > 16
    e = jpegamd.Encoder(w, h)
    try:
        e.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
        (f,), st = rgb_files(jpegamd, e, [rgb], dev, S420, 0, q)
    finally:
        e.close()
    assert f == m.file and st.entropy_bits == m.scan_bits


def device_tables(jpegamd, enc, tables):
    n = len(tables)
    freq = np.ascontiguousarray(np.stack(tables), np.uint64)
    bits, vals, nvals = np.zeros((n, 16), np.uint8), np.zeros((n, 256), np.uint8), np.zeros(n, np.int32)
    rc = jpegamd.lib.jpegamd_debug_optimal_huffman(enc._h, freq.ctypes.data, n, bits.ctypes.data, vals.ctypes.data, nvals.ctypes.data)
    assert rc == 0, rc
    return [(bits[i].tolist(), vals[i, :nvals[i]].tolist(), vals[i, nvals[i]:]) for i in range(n)]


def test_table_kernel_on_fibonacci_and_random_counts(jpegamd, dev, enc):
    tables = hf.count_tables()
    assert len(tables) % 4 != 0                                      # the last workgroup of the launch is not full
    got = device_tables(jpegamd, enc, tables)
    for f, (bits, vals, rest) in zip(tables, got):
        want_bits, want_vals, _ = hm.optimal_table(f)
        assert (bits, vals) == (want_bits, want_vals)
        assert not rest.any()
    assert device_tables(jpegamd, enc, tables[:1])[0][:2] == got[0][:2]


# ---- 5. counts ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_counts_are_the_models(jpegamd, oracle, dev, enc, sub):
    rgbs = [hf.content_rgb(200, 120, 0), hf.content_rgb(200, 120, 1)]
    for ri in (0, 5):
        models, _ = check_rgb(jpegamd, oracle, enc, dev, rgbs, sub, ri, 75)
        counts = np.zeros((2, 4, 256), np.uint64)
        assert jpegamd.lib.jpegamd_debug_huffman_counts(enc._h, counts.ctypes.data) == 0
        for c, m in zip(counts, models):
            assert (c.astype(np.int64) == m.counts).all(), (sub, ri)
        assert models[0].pad_blocks > 0 or sub == S444


# ---- 6. capacity ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ri", (0, 5))
def test_buffer_one_byte_too_small(jpegamd, oracle, dev, enc, ri):
    rgbs = gs.pictures(jpegamd, 72, 40, 2, seed=9)
    models = [hf.model(oracle, r, 75, S420, ri) for r in rgbs]
    big, small = sorted(range(2), key=lambda i: -len(models[i].file))
    assert len(models[big].file) > len(models[small].file)
    call = ms.PixelsCall(jpegamd, enc, rgbs, dev, S420, "rgb", ri, 75, cap=len(models[big].file) - 1)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == ERR_HUFF_CAPACITY
    sizes = call.sizes.cpu().tolist()
    files = gs.intact_files(call)                                    # nothing written past the capacity
    assert sizes[big] == 0 and sizes[small] == len(models[small].file) and files[small] == models[small].file
    check_rgb(jpegamd, oracle, enc, dev, rgbs, S420, ri, 75)         # the context is usable afterwards


# ---- 7. mode hygiene ------------------------------------------------------------------------------------------------------------------------------
def test_standard_after_optimized_is_todays_file(jpegamd, oracle, dev):
    rgb = hf.synth_rgb(72, 40, 5)
    e = jpegamd.Encoder(512, 64)
    try:
        for ri in (0, 3):
            std = hm.standard_file(oracle, rgb, 50, S420, ri)
            (before,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, ri, 50)
            e.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
            (opt,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, ri, 50)
            e.set_huffman(jpegamd.HUFFMAN_STANDARD)
            (after,), st = rgb_files(jpegamd, e, [rgb], dev, S420, ri, 50)
            assert before == after == std and opt == hf.model(oracle, rgb, 50, S420, ri).file and len(opt) < len(std)
        with pytest.raises(jpegamd.JpegAmdError):
            e.set_huffman(2)
    finally:
        e.close()


def test_mjpeg_functions_leave_the_shared_context_in_standard(jpegamd, oracle, dev):
    import jpegamd.mjpeg as mj
    rgb = hf.synth_rgb(72, 40, 6)
    t = torch.from_numpy(rgb).to(dev)
    for ri in (None, 4):
        want = hf.model(oracle, rgb, 50, S420, ri or 0).file
        std = hm.standard_file(oracle, rgb, 50, S420, ri or 0)
        assert mj.encode_tensor(t, 50, S420, restart_interval=ri, huffman="optimized") == want
        assert mj.encode_tensor(t, 50, S420, restart_interval=ri) == std                       # the shared context is back in STANDARD
        assert mj.encode_tensor_batch(t[None], 50, S420, restart_interval=ri, huffman="optimized") == [want]
        assert jpegamd.encode_tensor_batch(t[None], 50, S420, scan="interleaved", restart_interval=ri) == [std]
    planes = ms.derived_planes(rgb, S420)
    y, cb, cr = (torch.from_numpy(p).to(dev)[None] for p in planes)
    assert mj.encode_ycbcr_batch(y, cb, cr, 50, S420, huffman="optimized") == [hf.planes_model(oracle, planes, 50, S420, 0).file]
    assert mj.encode_ycbcr_batch(y, cb, cr, 50, S420) == [cm.memo(im.interleaved_ycbcr_file, oracle, *planes, 50, S420).file]
