"""The quantiser model (tests/quant_model.py) against the oracle, and the directed fixtures (tests/quant_fixtures.py) against the model
-- on the CPU.  Nothing here compares with the product's kernels; what comes from the library is the constants its debug entries expose."""
from __future__ import annotations

import numpy as np
import pytest

import quant_fixtures as qf
import quant_model as qm
import range_model as rm

KINDS = ("full", "ymap", "cmap")


def sample_blocks():
    """Low-amplitude, uniform-noise, flat and extreme blocks."""
    rng = np.random.default_rng(20264)
    low = np.clip(rng.integers(-100, 101, (768, 1)) + rng.integers(-4, 5, (768, 64)), -128, 127)
    mid = np.clip(rng.integers(-60, 61, (256, 1)) + rng.integers(-40, 41, (256, 64)), -128, 127)
    uni = rng.integers(-128, 128, (384, 64))
    flat = np.repeat(np.array([-128, -1, 0, 1, 127])[:, None], 64, axis=1)
    board = np.where(np.indices((8, 8)).sum(0) % 2, 127, -128).reshape(1, 64)
    return np.concatenate([low, mid, uni, flat, board, -board - 1])


def tile_walk(m, nblk=32, ballot_lanes=64, flag_thr_of_half0=False, one_round=False, todo_cap=None, grp_thr_scale=1.0):
    """The kernel's WAVE-UNIFORM decisions over one tile, from the per-site model `m` of its blocks (evaluate() of [nblk, 64]): the
    group_alive ballots, the flag test's ballot against flag_thr, and the fallback's rounds and batches -> (events, values int64 [nblk, 64]).
    Lanes b >= nblk shadow the last block; their flags are dropped.  With the defaults this is the kernel as written, and must give
    (m.flags.sum(), m.value) on any tile if the thresholds are safe.  The keyword arguments each switch ONE decision to a plausible
    mistake (a restatement of sections 3 and 4 of k_tile_encode, kept here beside its only user: edit it with the kernel) -- the ballot over half the wave, flag_thr read without its lane-half offset, a fallback of one round, a batch list cut to
    four events, a scaled grp_thr -- so that a host test can show which fixtures would notice."""
    c = m.consts
    lane_blk = np.minimum(np.arange(32), nblk - 1)
    hi, fr = m.hi_max[lane_blk], m.fract[lane_blk].reshape(32, 4, 2, 8)                 # [b, G, h(, j)]
    halves = (0, 1) if ballot_lanes == 64 else (0,)
    values = np.zeros((32, 4, 2, 8), np.int64)
    flagged = np.zeros((32, 4, 2, 8), bool)
    for G in range(4):
        if G and not any((hi[:, G, h] >= np.float32(c.grp_thr[G, h] * np.float32(grp_thr_scale))).any() for h in halves):
            continue                                                                     # a dead group: nothing is appended, i.e. zeros
        values[:, G] = m.fast[lane_blk].reshape(32, 4, 2, 8)[:, G]
        if any((fr[:, G, h].min(axis=1) <= np.float64(c.flag_thr[G, 0 if flag_thr_of_half0 else h])).any() for h in (0, 1)):
            flagged[:, G] = m.flags[lane_blk].reshape(32, 4, 2, 8)[:, G]
    flagged[nblk:] = False
    ref = m.ref[lane_blk].reshape(32, 4, 2, 8)
    events = 0
    # a lane's sites in the order of its flag bits: site 8 G + j of lane 32 h + b
    bits = {(h, b): [(G, j) for G in range(4) for j in range(8) if flagged[b, G, h, j]] for h in (0, 1) for b in range(32)}
    while any(bits.values()):
        todo = [ln for ln in sorted(bits, key=lambda hb: 32 * hb[0] + hb[1]) if bits[ln]]
        served = todo if todo_cap is None else todo[:todo_cap]
        for (h, b) in todo:
            G, j = bits[(h, b)][0]
            values[b, G, h, j] = ref[b, G, h, j] if (h, b) in served else 0              # (an unserved lane writes back the cleared register)
            bits[(h, b)] = [] if one_round else bits[(h, b)][1:]
        events += len(served)
    return events, values.reshape(32, 64)[:nblk]


@pytest.mark.parametrize("table", ["luma", "chroma"])
def test_unflagged_fast_values_are_the_references_at_every_quality(jpegamd, oracle, table):
    """For every quality 1 .. 100: a site the model does not flag has the reference's value; a DC is never flagged; and a block whose hi
    sums of a group all lie below grp_thr has neither a flag nor a non-zero reference value there (so skipping it is right)."""
    P = sample_blocks()
    flagged = differ = 0
    for q in range(1, 101):
        m = qm.evaluate(jpegamd, oracle, P, table, q)
        bad = np.argwhere(~m.flags & (m.fast != m.ref))
        assert not len(bad), (table, q, bad[:4].tolist())
        assert not m.flags[:, 0].any() and np.array_equal(m.fast[:, 0], m.ref[:, 0])
        dead = qm.dead_groups(m)
        assert not dead[:, 0].all()
        in_dead = np.repeat(dead, 16, axis=1)
        in_dead[:, :16] = False                                            # (group 0 is never skipped)
        assert not (m.flags & in_dead).any() and not ((m.ref != 0) & in_dead).any(), (table, q)
        assert np.array_equal(m.mask != 0, m.flags.any(axis=1))
        flagged += int(m.flags.sum())
        differ += int((m.flags & (m.fast != m.ref)).sum())
    assert flagged > 1000 and differ > 50                                  # (the band is there for a reason)


def test_single_rounding_helpers():
    """fma32 rounds once where float64-then-float32 would round twice; fract_le decides at the threshold exactly."""
    f32 = np.float32
    a, b = f32(2.0 ** -24 * (1.0 + 2.0 ** -12)), f32(1.0 - 2.0 ** -12 + 2.0 ** -24)      # a b = 2^-24 (1 + 2^-36), exactly
    c = f32(1.0 + 2.0 ** -22)                                              # a b + c lies 2^-60 above the float32 tie 1 + 2^-22 + 2^-24 ...
    s64 = np.float64(a) * np.float64(b) + np.float64(c)
    assert np.float64(a) * np.float64(b) == 2.0 ** -24 + 2.0 ** -60 and s64 == 1.0 + 2.0 ** -22 + 2.0 ** -24      # ... which the float64 sum lands on
    st = {}
    got = qm.fma32(np.array([a]), np.array([b]), np.array([c]), st)[0]
    assert st["fma_exact"] == 1 and got == f32(1.0 + 2.0 ** -22 + 2.0 ** -23) and f32(s64) == f32(1.0 + 2.0 ** -22)       # (rounded twice: to even, down)
    thr = f32(0.001)
    zc = np.array([f32(3.0) + thr, np.nextafter(f32(3.0) + thr, f32(4)), f32(-2.0) + thr], f32)
    want = [(float(z) - np.floor(float(z))) <= float(thr) for z in zc]     # (exact in float64: 24-bit values within one binade step)
    assert list(qm.fract_le(zc, thr)) == want


@pytest.mark.parametrize("kind", KINDS)
def test_every_fixture_sits_where_it_claims(jpegamd, oracle, kind):
    s = qf.fixture_set(jpegamd, oracle, kind)
    names = [f.name for f in s.fixtures]
    assert len(set(names)) == len(names) == 66
    for G in (1, 2, 3):
        for h in (0, 1):
            for b in (0, 31):
                assert f"live_g{G}h{h}_b{b}" in names and f"dead_g{G}h{h}_b{b}" in names
    assert {f"lane{ln}" for ln in qf.FLAG_LANES} | {f"count{n}" for n in (1, 4, 5, 8, 9)} <= set(names)
    by_name = {f.name: f for f in s.fixtures}
    assert all(f.quality == 100 for f in s.fixtures if f.name.endswith("_q100")) and sum(f.name.endswith("_q100") for f in s.fixtures) == 15
    assert by_name["three_sites"].quality == 100 and all(f.quality == qf.SKIP_QUALITY for f in s.fixtures if "live" in f.name or "dead" in f.name)
    for f in s.fixtures:
        m = qf.verify(jpegamd, oracle, f)
        if kind != "full":
            assert np.isin(f.tile + 128, s.values).all(), f.name            # every sample has a preimage under the map
        # the kernel's wave-uniform decisions, walked over the tile and over the ragged tile of its key block, give the model's answer
        assert tile_walk(m)[0] == m.flags.sum() and np.array_equal(tile_walk(m)[1], m.value), f.name
        key = qm.evaluate(jpegamd, oracle, f.tile[f.key:f.key + 1], f.table, f.quality)
        ev, val = tile_walk(key, nblk=1)
        assert ev == key.flags.sum() and np.array_equal(val, key.value), f.name
    for n, lanes in qf.COUNT_LANES.items():
        assert len(lanes) == n and len({ln & 31 for ln in lanes}) == n
    su = qf.summary(jpegamd, oracle, kind)
    assert su["luma"]["differ"] >= 16 and su["chroma"]["differ"] >= 16 and su["luma"]["ties"] >= 1 and su["chroma"]["ties"] >= 1, su


@pytest.mark.parametrize("kind", KINDS)
def test_planes_hold_the_tiles(jpegamd, oracle, kind):
    s = qf.fixture_set(jpegamd, oracle, kind)
    for q in s.qualities():
        fx = s.of_quality(q)
        p, r = s.plane(q), s.plane(q, 264)
        assert p.shape == (8 * len(fx), 256) and r.shape == (8 * len(fx), 264) and np.array_equal(r[:, :256], p)
        blocks, ragged = qm.plane_blocks(p).reshape(len(fx), 32, 64), qm.plane_blocks(r).reshape(len(fx), 33, 64)
        for i, f in enumerate(fx):
            assert np.array_equal(blocks[i], f.tile) and np.array_equal(ragged[i, 32], f.tile[f.key]) and f.tile[f.key].any(), f.name
        if kind != "full":
            pre = qf.preimage(kind)
            table = rm.luma_table() if kind == "ymap" else rm.chroma_table()
            assert np.array_equal(table[pre[r]], r) and pre[r].min() >= 16   # the stored plane is limited range, and maps onto the fixture plane


def test_each_decision_gone_wrong_moves_some_fixture(jpegamd, oracle):
    """tile_walk with ONE wave-uniform decision changed at a time: for each there are fixtures whose event count or coefficients come out
    different from the model's -- the tiles that pin that decision.  (The same changes made in the kernel itself are what the GPU tests of
    tests/test_gpu_quantiser.py must catch; this shows on the CPU that the fixtures are placed to do so.)"""
    s = qf.fixture_set(jpegamd, oracle, "full")
    models = {f.name: qm.evaluate(jpegamd, oracle, f.tile, f.table, f.quality) for f in s.fixtures}

    def moved(**kw):
        out = set()
        for name, m in models.items():
            ev, val = tile_walk(m, **kw)
            if ev != m.flags.sum() or not np.array_equal(val, m.value):
                out.add(name)
        return out

    assert not moved()
    assert "own_half_h1" in moved(flag_thr_of_half0=True)
    assert {f"live_g{G}h1_b{b}" for G in (1, 2, 3) for b in (0, 31)} <= moved(ballot_lanes=32)
    assert {"two_sites_one_group", "two_sites_two_groups", "three_sites"} <= moved(one_round=True)
    assert {"count5", "count8", "count9", "count5_q100", "count8_q100", "count9_q100"} <= moved(todo_cap=4)
    assert not {"count1", "count4", "count1_q100", "count4_q100"} & moved(todo_cap=4)
    assert {f"live_g{G}h{h}_b{b}" for G in (1, 2, 3) for h in (0, 1) for b in (0, 31)} <= moved(grp_thr_scale=1.5)
