"""The tile kernel's quantiser on the GPU, decision by decision: which groups a tile skips, which coefficients it flags, and what the
exact-order fallback writes back -- against the CPU model of tests/quant_model.py (the flagged set, block for block, and the number
of fallback events) and the oracle (the coefficients and the file bytes), on the directed tiles of tests/quant_fixtures.py and on every
quality 1 .. 100 of both tables.  Never product against product.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import quant_fixtures as qf
import quant_model as qm
import range_model as rm
from gpu_support import CBCR, PLANES, S422, S444, YUYV, YccBatch, block_rows_reversed, dev, finish_files, rows_for, upload     # noqa: F401
from gpu_support import encode_gray_planes as encode_gray
from gpu_support import gray_bmp_sized as gray_bmp
from gpu_support import ycc_file as expected

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WIDTHS = (256, 264)                                              # whole tiles; and a ragged tile of one block behind every whole one


@pytest.fixture(scope="module")
def full(jpegamd, oracle):
    return qf.fixture_set(jpegamd, oracle, "full")


def gray_file(oracle, plane, q):
    return cm.memo(cm.gray_file, oracle, plane, q)


def flags_of(jpegamd, oracle, plane, table, q) -> int:
    """The model's number of fallback events over the active blocks of a plane (every block of the padded picture)."""
    return int(qm.plane_model(jpegamd, oracle, plane, table, q).flags.sum())


def differ_of(jpegamd, oracle, plane, table, q) -> int:
    """... and of those events, the ones whose fast value is not the reference's: what the fallback is for."""
    m = qm.plane_model(jpegamd, oracle, plane, table, q)
    return int((m.flags & (m.fast != m.ref)).sum())


def flat_like(plane, value=128):
    return np.full_like(plane, value)


def encode_ycc(jpegamd, enc, planes, dev, layout, q, **kw):
    """4:4:4 YCbCr pictures through jpegamd_encode_ycbcr_batch_async (kw: YccBatch's, such as a sample range) -> (files, Stats)."""
    return finish_files(enc, YccBatch(jpegamd, enc, planes, dev, S444, layout, quality=q, **kw))


# ---- 1. the taps build: coefficients and the flagged set, block for block -----------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
def test_taps_build_flags_exactly_the_models_sites(jpegamd, oracle, dev, full, width):
    """jpegamd_debug_stages over every fixture plane as ORDER_GRAY, through the dword loader and through the byte loader (stride + 1, the
    pointer shifted by 1): quant_zigzag is the oracle's, exact_mask is the model's mask."""
    enc = jpegamd.Encoder(width + 8, max(full.plane(q).shape[0] for q in full.qualities()))
    for q in full.qualities():
        p = full.plane(q, width)
        h, w = p.shape
        want_zz = oracle.stages(gray_bmp(p), q)["zigzag"]
        m = qm.plane_model(jpegamd, oracle, p, "luma", q)
        assert np.array_equal(m.value, want_zz.astype(np.int64)), q          # (the model's own values: the reference's where flagged)
        n = len(want_zz)
        for stride, shift in ((w, 0), (w + 1, 1)):
            t, ptr = upload(p, dev, stride, shift)
            zz = torch.zeros(n * 64, dtype=torch.int16, device=dev)
            mask = torch.zeros(n, dtype=torch.int64, device=dev)
            enc.debug_stages(jpegamd.Encoder.image(ptr, w, h, stride, False, jpegamd.ORDER_GRAY, q), 0, zz.data_ptr(), mask.data_ptr())
            got_zz, got_mask = zz.cpu().numpy().reshape(n, 64), mask.cpu().numpy().view(np.uint64)
            bad = np.nonzero((got_zz != want_zz).any(axis=1))[0]
            assert not len(bad), (q, width, shift, "blocks (tile, lane) whose coefficients differ", [divmod(int(i), w // 8) for i in bad[:8]])
            bad = np.nonzero(got_mask != m.mask)[0]
            assert not len(bad), (q, width, shift, "blocks (tile, lane) whose flagged set differs",
                                  [(divmod(int(i), w // 8), hex(int(got_mask[i])), hex(int(m.mask[i]))) for i in bad[:8]])


# ---- 2. the hot path, luma tables -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_hot_path_luma_bytes_and_fallback_count(jpegamd, oracle, dev, full, pipeline):
    """jpegamd_encode_async and a batch of 3 (the hot-path instantiation: a dead upper half never runs its lo chain): the oracle's bytes,
    and Stats.exact_fallbacks is the model's flag count over the active blocks."""
    for width in WIDTHS:
        enc = jpegamd.Encoder(width, rows_for(3, max(full.plane(q).shape[0] for q in full.qualities())))
        enc.set_pipeline(getattr(jpegamd, pipeline))
        for q in full.qualities():
            p = full.plane(q, width)
            flags = flags_of(jpegamd, oracle, p, "luma", q)
            assert flags > 0 or q == qf.SKIP_QUALITY                     # (the group-skip tiles have no flagged site: their count is 0)
            files, st = encode_gray(jpegamd, enc, [p], dev, q)
            assert st.exact_fallbacks == flags, (q, width, "single", st.exact_fallbacks, flags)
            assert files == [gray_file(oracle, p, q)], (q, width, "single")
            r = block_rows_reversed(p)
            files, st = encode_gray(jpegamd, enc, [p, r, p], dev, q)
            assert st.exact_fallbacks == 2 * flags + flags_of(jpegamd, oracle, r, "luma", q), (q, width, "batch", st.exact_fallbacks, flags)
            assert files == [gray_file(oracle, x, q) for x in (p, r, p)], (q, width, "batch")
    assert sum(differ_of(jpegamd, oracle, full.plane(q), "luma", q) for q in full.qualities()) >= 16


# ---- 3. the hot path, chroma tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", [PLANES, CBCR])
def test_hot_path_chroma_bytes_and_fallback_count(jpegamd, oracle, dev, full, layout):
    """The fixture planes as Cb, then as Cr, of a 4:4:4 YCbCr picture whose other planes are flat (0 flags, by the model)."""
    for width in WIDTHS:
        enc = jpegamd.Encoder(width, rows_for(2, max(full.plane(q).shape[0] for q in full.qualities())))
        for q in full.qualities():
            p = full.plane(q, width)
            flat = flat_like(p)
            assert flags_of(jpegamd, oracle, flat, "luma", q) == 0 and flags_of(jpegamd, oracle, flat, "chroma", q) == 0
            flags = flags_of(jpegamd, oracle, p, "chroma", q)
            planes = [(flat, p, flat), (flat, flat, p)]
            files, st = encode_ycc(jpegamd, enc, planes, dev, layout, q)
            assert st.exact_fallbacks == 2 * flags, (q, width, st.exact_fallbacks, flags)
            assert files == [expected(oracle, x, q, S444) for x in planes], (q, width)
    assert sum(differ_of(jpegamd, oracle, full.plane(q), "chroma", q) for q in full.qualities()) >= 16      # (what ran held the events the fallback is for)


# ---- 4. the range-expanding instantiations --------------------------------------------------------------------------------------------
def limited_sets(jpegamd, oracle):
    """The fixture sets searched over the mapped values (the images of the limited-range maps: many full-range fixture values have no
    preimage), and the limited-range planes that range_model.expand maps onto their planes."""
    ys, cs = qf.fixture_set(jpegamd, oracle, "ymap"), qf.fixture_set(jpegamd, oracle, "cmap")
    return ys, cs, qf.preimage("ymap"), qf.preimage("cmap")


@pytest.mark.parametrize("layout", [PLANES, CBCR])
def test_expanding_instantiations_chroma_planes(jpegamd, oracle, dev, layout):
    """sample_range="limited": the same pictures, the stored planes chosen so that the map gives the fixture planes.  Count and bytes are
    those of the mapped planes."""
    ys, cs, ypre, cpre = limited_sets(jpegamd, oracle)
    for width in WIDTHS:
        enc = jpegamd.Encoder(width, rows_for(2, max(cs.plane(q).shape[0] for q in cs.qualities())))
        for q in cs.qualities():
            p = cs.plane(q, width)
            flat = flat_like(p)
            stored = [(ypre[flat], cpre[p], cpre[flat]), (ypre[flat], cpre[flat], cpre[p])]
            mapped = [rm.expand(x) for x in stored]
            assert all(np.array_equal(a, b) for m, x in zip(mapped, [(flat, p, flat), (flat, flat, p)]) for a, b in zip(m, x))
            flags = flags_of(jpegamd, oracle, p, "chroma", q)
            files, st = encode_ycc(jpegamd, enc, stored, dev, layout, q, sample_range=jpegamd.RANGE_LIMITED)
            assert st.exact_fallbacks == 2 * flags, (q, width, st.exact_fallbacks, flags)
            assert files == [expected(oracle, x, q, S444) for x in mapped], (q, width)
        assert sum(differ_of(jpegamd, oracle, cs.plane(q, width), "chroma", q) for q in cs.qualities()) >= 16


def _pad_rows(plane, rows, value=128):
    return np.ascontiguousarray(np.pad(plane, ((0, rows - plane.shape[0]), (0, 0)), constant_values=value))


@pytest.mark.parametrize("layout", [PLANES, YUYV])               # I422, and the packed plane
def test_expanding_instantiations_y_and_422(jpegamd, oracle, dev, layout):
    """4:2:2, limited range: the Y plane is two copies of the luma-map fixture plane side by side (through the plane loader for I422, the
    pair loader for YUYV), Cb and Cr the chroma-map fixture planes (the plane loader, the quad loader)."""
    ys, cs, ypre, cpre = limited_sets(jpegamd, oracle)
    q = 90
    for width in WIDTHS:
        yp, cp = ys.plane(q, width), cs.plane(q, width)
        rows = max(yp.shape[0], cp.shape[0])
        yp, cp = _pad_rows(yp, rows), _pad_rows(cp, rows)
        y, cb, cr = np.ascontiguousarray(np.hstack([yp, yp])), cp, block_rows_reversed(cp)
        stored = (ypre[y], cpre[cb], cpre[cr])
        mapped = rm.expand(stored)
        assert all(np.array_equal(a, b) for a, b in zip(mapped, (y, cb, cr)))
        flags = flags_of(jpegamd, oracle, y, "luma", q) + flags_of(jpegamd, oracle, cb, "chroma", q) + flags_of(jpegamd, oracle, cr, "chroma", q)
        enc = jpegamd.Encoder(2 * width, rows_for(1, rows))
        b = YccBatch(jpegamd, enc, [stored], dev, S422, layout, quality=q, sample_range=jpegamd.RANGE_LIMITED)
        st = enc.finish()
        res = b.results()
        assert all(ok for _, ok in res)
        assert st.exact_fallbacks == flags and flags > 0, (width, st.exact_fallbacks, flags)
        assert [f for f, _ in res] == [expected(oracle, mapped, q, S422)], width


# ---- 5. every quality, both tables ----------------------------------------------------------------------------------------------------
def sweep_planes():
    rng = np.random.default_rng(20263)
    noise = rng.integers(0, 256, (16, 264), np.uint8)
    low = (128 + rng.integers(-100, 101, (2, 33)).repeat(8, axis=0).repeat(8, axis=1) + rng.integers(-4, 5, (16, 264))).clip(0, 255).astype(np.uint8)
    return noise, low


@pytest.mark.parametrize("first", [1, 26, 51, 76])
def test_every_quality_both_tables(jpegamd, oracle, dev, first):
    """One context for 25 qualities in turn (the tables are derived again between calls): a noise plane and a low-amplitude plane, 264 x 16,
    as GRAY and as Cb.  The oracle's / the chroma model's bytes, and the model's fallback count."""
    noise, low = sweep_planes()
    flat = flat_like(noise)
    enc = jpegamd.Encoder(264, rows_for(2, 16))
    for q in range(first, first + 25):
        want = sum(flags_of(jpegamd, oracle, p, "luma", q) for p in (noise, low))
        files, st = encode_gray(jpegamd, enc, [noise, low], dev, q)
        assert st.exact_fallbacks == want, (q, "luma", st.exact_fallbacks, want)
        assert files == [gray_file(oracle, p, q) for p in (noise, low)], (q, "luma")
        want = sum(flags_of(jpegamd, oracle, p, "chroma", q) for p in (noise, low))
        planes = [(flat, noise, flat), (flat, low, flat)]
        files, st = encode_ycc(jpegamd, enc, planes, dev, PLANES, q)
        assert st.exact_fallbacks == want, (q, "chroma", st.exact_fallbacks, want)
        assert files == [expected(oracle, x, q, S444) for x in planes], (q, "chroma")
