"""The premise of tests/test_gpu_stash_sequence.py, on the CPU: the picture of tests/stash_sequence.py makes every wave of k_tile_encode
code several tiles, with and without an exact-order event in turn -- by the model of tests/quant_model.py, not by the product."""
from __future__ import annotations

import numpy as np

import quant_model as qm
import stash_sequence as ss


def test_launch_waves_come_from_the_source():
    assert ss.launch_waves() == 512 * 8                       # (what the kernel is built with today; the picture follows the source)


def test_picture_alternates_tiles_with_and_without_events(jpegamd, oracle):
    p = ss.picture(jpegamd, oracle)
    h, w = p.plane.shape
    tiles = h // 8 * 2
    assert w == 512 and h % 8 == 0 and h <= 65535 and tiles == len(p.names) == len(p.has_event)
    assert tiles >= 3 * p.waves and tiles % (2 * ss.PATTERN) == 0      # every wave of a full launch codes three tiles on average
    # the tiles the sequence is named for have events, the flat tile and (some of) the dead_* tiles have none -- at the picture's quality
    assert set(ss.EVENT_TILES) <= set(p.event_kinds), p.event_kinds
    assert "flat" in p.none_kinds and any(n.startswith("dead_") for n in p.none_kinds), p.none_kinds
    assert all(n in p.names for n in ss.EVENT_TILES) and "flat" in p.names
    share = p.has_event.mean()
    print(f"quality {p.quality}: {tiles} tiles, {100 * share:.1f} % with an event, {p.events} events by the model")
    assert 0.25 <= share <= 0.75, share
    # (neighbours in tile order, the order of the hand-out: side by side or across a row end)
    after_none = int((p.has_event[1:] & ~p.has_event[:-1]).sum())      # a tile with an event behind one without
    after_event = int((~p.has_event[1:] & p.has_event[:-1]).sum())
    print(f"event after none {after_none}, none after event {after_event}")
    assert after_none >= 1000 and after_event >= 1000, (after_none, after_event)
    # the recorded total is the model's count over the blocks of the picture itself (two patterns' worth, PATTERN block rows: the rest
    # are copies)
    two = p.plane[:8 * ss.PATTERN]
    copies = tiles // (2 * ss.PATTERN)
    assert np.array_equal(p.plane, np.tile(two, (copies, 1)))
    m = qm.plane_model(jpegamd, oracle, two, "luma", p.quality)
    assert int(m.flags.sum()) * copies == p.events and p.events > 0
    per_tile = m.flags.reshape(2 * ss.PATTERN, 32, 64).any(axis=(1, 2))        # (raster block order of a 64-block row = tile order)
    assert np.array_equal(per_tile, p.has_event[:2 * ss.PATTERN])
