"""Directed fixtures for the tile kernel's quantiser: its group-skip, flag and exact-order-fallback decisions -- TEST INFRASTRUCTURE ONLY.

Every fixture is ONE tile: 32 blocks of one block row, 256 x 8 samples, flat (128) but for the blocks the fixture is about.  The blocks
come from a seeded, deterministic search through the CPU model (tests/quant_model.py) over at most CAP candidate blocks per pool;
nothing is stored in files.  A search that comes up empty raises: it is an error, never a skip.

Two candidate pools, CAP blocks each:
  low     a level in -100 .. 100 plus uniform noise in -4 .. 4 per sample (low amplitude: what the fallback fixtures are drawn from)
  basis   one DCT basis function of groups 1 .. 3 at 0.30 .. 0.80 quantiser steps of the Q=50 luma table, plus noise in -1 .. 1 (the
          group-skip fixtures: a group's hi sums around its zero threshold while the other groups stay quiet)
A fixture set may be restricted to a set of sample values (every candidate is snapped to the nearest allowed value): the images of the
limited-range maps of tests/range_model.py, for the pictures that reach the kernel through its range expansion -- 36 of the 256 luma
values and 31 of the chroma values have no preimage under those maps, so the limited-range fixtures are searched over mapped values
instead of being derived from the full-range ones.

The group-skip fixtures sit at Q=50.  The fallback fixtures are searched at Q=90 first and at Q=100 where Q=90 has no candidate; the
quality that served is recorded in the fixture.  The lane, count, both-lanes and each-group tiles are made at Q=100 as well (`*_q100`);
a search that fails there raises LookupError, which nothing catches.  Each fixture carries its claims, and verify() asserts them from the model."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import quant_model as qm
import range_model as rm

CAP = 32768                                   # candidate blocks per pool
SKIP_QUALITY = 50
FALLBACK_QUALITIES = (90, 100)
# flag_thr of lane half 1 exceeds that of lane half 0 in group 0 of the luma table at Q=92 and Q=95 .. 100 alone, by 5 % at Q=92 / 95 and
# by 1.6 % above (a band the low pool's lattice of sums never hits at Q=100): the fixture for that case is searched at Q=95 as well
OWN_HALF_EXTRA = (95,)
FLAG_LANES = (0, 15, 16, 31, 32, 47, 48, 63)
# flagged lanes of the count tiles (lane = 32 h + b; the two lanes of a block are never both listed: every block has one flag).  Events
# are handled in lane order, four per batch: 4 / 5 and 8 / 9 straddle the batch boundary.
COUNT_LANES = {1: (40,), 4: (0, 31, 47, 48), 5: (8, 15, 16, 32, 63), 8: (0, 15, 16, 31, 33, 46, 49, 62), 9: (1, 14, 17, 30, 32, 40, 47, 48, 63)}


def value_set(kind: str):
    """Allowed sample values of a fixture set: None (all of 0 .. 255), or the image of a limited-range map."""
    if kind == "full":
        return None
    return np.unique(rm.luma_table() if kind == "ymap" else rm.chroma_table()).astype(np.int64)


def preimage(kind: str) -> np.ndarray:
    """uint8 [256]: for every value in the image of the map of `kind`, a limited-range sample that maps onto it (0 elsewhere)."""
    t = rm.luma_table() if kind == "ymap" else rm.chroma_table()
    inv = np.zeros(256, np.uint8)
    for v in range(255, 15, -1):
        inv[t[v]] = v
    return inv


def _snap(P, values):
    if values is None:
        return P
    near = np.array([values[np.argmin(np.abs(values - v))] for v in range(256)], np.int64)
    return near[P + 128] - 128


def low_pool(values=None, seed=20261):
    rng = np.random.default_rng(seed)
    return _snap(np.clip(rng.integers(-100, 101, (CAP, 1)) + rng.integers(-4, 5, (CAP, 64)), -128, 127), values)


def basis_pool(oracle, values=None, seed=20262):
    rng = np.random.default_rng(seed)
    qt = qm.table_of(oracle, "luma", SKIP_QUALITY).astype(np.float64)
    x = np.arange(8)
    cosm = np.cos((2 * x[:, None] + 1) * np.arange(8)[None, :] * np.pi / 16)       # [x][u]
    P = np.zeros((CAP, 64), np.int64)
    for i in range(CAP):
        G, h = 1 + (i % 6) // 2, i % 2
        k = int(qm.ZZ[16 * G + 8 * h + rng.integers(0, 8)])
        u, v = divmod(k, 8)
        F = qt[k] * rng.uniform(0.30, 0.80) * (1 if rng.integers(0, 2) else -1)
        b = 0.25 * (0.5 ** 0.5 if u == 0 else 1.0) * (0.5 ** 0.5 if v == 0 else 1.0) * F * np.outer(cosm[:, u], cosm[:, v])
        P[i] = np.clip(np.rint(b).astype(np.int64).reshape(64) + rng.integers(-1, 2, 64), -128, 127)
    return _snap(P, values)


def _tile(blocks_at):
    t = np.zeros((32, 64), np.int64)
    for b, blk in blocks_at.items():
        t[b] = blk
    return t


class FixtureSet:
    def __init__(self, jpegamd, oracle, kind="full"):
        self.jpegamd, self.oracle, self.kind = jpegamd, oracle, kind
        self.values = value_set(kind)
        self.fixtures = []
        self._models = {}
        self._used = set()
        self.low, self.basis = low_pool(self.values), basis_pool(oracle, self.values)
        self._skip()
        self._fallback()

    # ---- plumbing ---------------------------------------------------------------------------------------------------------------
    def model(self, pool: str, table: str, quality: int):
        key = (pool, table, quality)
        if key not in self._models:
            self._models[key] = qm.evaluate(self.jpegamd, self.oracle, getattr(self, pool), table, quality)
        return self._models[key]

    def add(self, name, quality, table, blocks_at, key, **claims):
        self.fixtures.append(SimpleNamespace(name=name, quality=quality, table=table, tile=_tile(blocks_at), key=key, claims=claims))

    def pick(self, mask, count=1, what="", pool="low"):
        """The first `count` candidates of `mask` (over `pool`) that no fixture of this set uses yet."""
        idx = [int(i) for i in np.nonzero(mask)[0] if (pool, int(i)) not in self._used][:count]
        if len(idx) < count:
            raise LookupError(f"{what}: {len(idx)} of {count} candidates among {CAP}")
        self._used.update((pool, i) for i in idx)
        return idx

    def at_first_quality(self, name, fn, qualities=FALLBACK_QUALITIES):
        """fn(quality) at Q=90, then at Q=100: the first quality that has the candidates serves, and is what the fixture records."""
        missed = []
        for q in qualities:
            try:
                return fn(q)
            except LookupError as e:
                missed.append(f"Q={q}: {e}")
        raise RuntimeError(f"fixture search came up empty ({self.kind} values): {name}: {missed}")

    # ---- group skip (Q=50, luma table) ----------------------------------------------------------------------------------------------
    def _skip(self):
        q = SKIP_QUALITY
        m = self.model("basis", "luma", q)
        thr = m.consts.grp_thr
        dead = qm.dead_groups(m)
        nz = (m.ref.reshape(-1, 4, 16) != 0).any(axis=2)
        for G in (1, 2, 3):
            for h in (0, 1):
                coef = np.abs(m.ref[:, 16 * G + 8 * h:16 * G + 8 * h + 8])
                live = (coef.sum(axis=1) == 1) & (m.hi_max[:, G, h] >= thr[G, h]) & (m.hi_max[:, G, 1 - h] < thr[G, 1 - h])
                if not live.any() or not dead[:, G].any():
                    raise RuntimeError(f"fixture search came up empty ({self.kind} values): group {G} half {h} among {CAP} candidates")
                i_live = int(np.nonzero(live)[0][np.argmin(m.hi_max[live, G, h])])
                # the dead block: the whole group strictly below its thresholds, and of those the largest hi sum in this half
                i_dead = int(np.nonzero(dead[:, G])[0][np.argmax(m.hi_max[dead[:, G], G, h])])
                for b in (0, 31):
                    self.add(f"live_g{G}h{h}_b{b}", q, "luma", {b: self.basis[i_live]}, b, live=(G, h, b))
                    self.add(f"dead_g{G}h{h}_b{b}", q, "luma", {b: self.basis[i_dead]}, b, dead=(G, b))
        combos = (("g2_alive_g3_dead", nz[:, 2] & ~dead[:, 2] & dead[:, 3], (False, True)),
                  ("g3_alive_g2_dead", nz[:, 3] & ~dead[:, 3] & dead[:, 2], (True, False)),
                  ("g1_alive_upper_dead", nz[:, 1] & ~dead[:, 1] & dead[:, 2] & dead[:, 3], (True, True)))
        for name, mask, upper_dead in combos:
            try:
                i = self.pick(mask, 1, name, pool="basis")[0]
            except LookupError as e:
                raise RuntimeError(f"fixture search came up empty ({self.kind} values): {e}")
            self.add(name, q, "luma", {13: self.basis[i]}, 13, upper_dead=upper_dead, nonzero_group=1 if name.startswith("g1") else int(name[1]))

    # ---- the exact-order fallback (Q=90, else Q=100) -----------------------------------------------------------------------------------
    def _counts(self, table, q):
        m = self.model("low", table, q)
        gh = m.flags.reshape(-1, 4, 2, 8).sum(axis=3)                  # flags per (group, lane half)
        return m, gh, gh.sum(axis=1), m.flags.sum(axis=1)               # ..., per lane half, per block

    def _fallback(self):
        def singles(q, lanes, name):
            """One block with exactly one flagged site per listed lane."""
            m, gh, lane, total = self._counts("luma", q)
            at = {}
            for ln in lanes:
                h, b = ln >> 5, ln & 31
                at[b] = self.low[self.pick((total == 1) & (lane[:, h] == 1), 1, name)[0]]
            return q, at

        for ln in FLAG_LANES:
            q, at = self.at_first_quality(f"lane{ln}", lambda q: singles(q, (ln,), f"lane{ln}"))
            self.add(f"lane{ln}", q, "luma", at, ln & 31, lanes=(ln,))
        for n, lanes in COUNT_LANES.items():
            q, at = self.at_first_quality(f"count{n}", lambda q: singles(q, lanes, f"count{n}"))
            self.add(f"count{n}", q, "luma", at, lanes[0] & 31, lanes=lanes)

        def lane_sites(q, nsites, ngroups, name):
            m, gh, lane, total = self._counts("luma", q)
            for h in (1, 0):
                groups = (gh[:, :, h] > 0).sum(axis=1)
                try:
                    return q, h, self.pick((total == nsites) & (lane[:, h] == nsites) & (groups == ngroups), 1, name)[0]
                except LookupError:
                    pass
            raise LookupError(f"{name}: no candidate among {CAP}")

        for name, nsites, ngroups, only in (("two_sites_one_group", 2, 1, None), ("two_sites_two_groups", 2, 2, None), ("three_sites", 3, None, 100)):
            def fn(q, nsites=nsites, ngroups=ngroups, name=name, only=only):
                if only and q != only:
                    raise LookupError(f"{name} is asked for at Q={only}")
                if ngroups is None:
                    for ng in (2, 3, 1):
                        try:
                            return lane_sites(q, nsites, ng, name)
                        except LookupError:
                            pass
                    raise LookupError(f"{name}: no candidate among {CAP}")
                return lane_sites(q, nsites, ngroups, name)
            q, h, i = self.at_first_quality(name, fn)
            self.add(name, q, "luma", {7: self.low[i]}, 7, lane_sites=(32 * h + 7, nsites, ngroups))

        def both(q):
            m, gh, lane, total = self._counts("luma", q)
            return q, self.pick((lane[:, 0] == 1) & (lane[:, 1] == 1), 1, "both_lanes")[0]
        q, i = self.at_first_quality("both_lanes", both)
        self.add("both_lanes", q, "luma", {21: self.low[i]}, 21, lanes=(21, 53))

        def each_group(q):
            m, gh, lane, total = self._counts("luma", q)
            return q, {3 + 8 * G: self.low[self.pick((total == 1) & (gh[:, G].sum(axis=1) == 1), 1, f"each_group: group {G}")[0]] for G in range(4)}
        q, at = self.at_first_quality("each_group", each_group)
        self.add("each_group", q, "luma", at, 27, flagged_groups=(0, 1, 2, 3))

        # the flag test's ballot against flag_thr[G][h]: the ONLY flagged site of the tile's group G sits in lane half h, and every
        # fraction of the block's group-G sites lies above the OTHER half's flag_thr: the ballot passes by this half's threshold alone
        def own_half(q, h):
            m, gh, lane, total = self._counts("luma", q)
            ft = m.consts.flag_thr
            fr = m.fract.reshape(-1, 4, 2, 8)
            for G in range(4):
                if not ft[G, h] > ft[G, 1 - h]:
                    continue
                mask = (gh[:, G, h] >= 1) & (fr[:, G].min(axis=(1, 2)) > np.float64(ft[G, 1 - h]))
                try:
                    return q, G, self.pick(mask, 1, f"own_half h{h}")[0]
                except LookupError:
                    pass
            raise LookupError(f"own_half h{h}: no candidate among {CAP}")
        for h in (0, 1):
            q, G, i = self.at_first_quality(f"own_half_h{h}", lambda q: own_half(q, h), FALLBACK_QUALITIES + OWN_HALF_EXTRA)
            self.add(f"own_half_h{h}", q, "luma", {5: self.low[i]}, 5, own_half=(G, h, 5))

        # the coefficients the fallback exists for: flagged, and the fast value is NOT the reference's
        for table in ("luma", "chroma"):
            def differ(q, table=table):
                m = self.model("low", table, q)
                d = (m.flags & (m.fast != m.ref)).any(axis=1)
                return q, self.pick(d, 16, f"differ_{table}")
            q, idx = self.at_first_quality(f"differ_{table}", differ)
            # (16 blocks, spread over the tile: every quarter of each lane half holds some)
            self.add(f"differ_{table}", q, table, {2 * j + (j & 1): self.low[i] for j, i in enumerate(idx)}, 0, differ=16)

            def ties(q, table=table):
                m = self.model("low", table, q)
                return q, self.pick((m.flags & m.tie & (m.fast != m.ref)).any(axis=1), 1, f"tie_{table}")
            q, idx = self.at_first_quality(f"tie_{table}", ties)
            self.add(f"tie_{table}", q, table, {30: self.low[idx[0]]}, 30, tie=1)

        # Lane delivery, the batch-of-four boundaries, both lanes of a block and the write-back per group are found at Q=90 above; the
        # same tiles are made at Q=100 as well (every quantiser step 1: other constants, many more flags to choose from)
        for ln in FLAG_LANES:
            self.add(f"lane{ln}_q100", 100, "luma", singles(100, (ln,), f"lane{ln}_q100")[1], ln & 31, lanes=(ln,))
        for n, lanes in COUNT_LANES.items():
            self.add(f"count{n}_q100", 100, "luma", singles(100, lanes, f"count{n}_q100")[1], lanes[0] & 31, lanes=lanes)
        self.add("both_lanes_q100", 100, "luma", {21: self.low[both(100)[1]]}, 21, lanes=(21, 53))
        self.add("each_group_q100", 100, "luma", each_group(100)[1], 27, flagged_groups=(0, 1, 2, 3))

    # ---- planes -------------------------------------------------------------------------------------------------------------------
    def qualities(self):
        return sorted({f.quality for f in self.fixtures})

    def of_quality(self, quality):
        return [f for f in self.fixtures if f.quality == quality]

    def plane(self, quality, width=256) -> np.ndarray:
        """uint8 [8 T, width]: the tiles of this quality's fixtures stacked, one block row each.  width 264: a 33rd block per row, a copy
        of the fixture's key block -- every block row then ends in a ragged tile of one active block (31 lanes shadow it)."""
        assert width in (256, 264)
        rows = []
        for f in self.of_quality(quality):
            t = f.tile if width == 256 else np.concatenate([f.tile, f.tile[f.key:f.key + 1]])
            rows.append((t.reshape(-1, 8, 8).transpose(1, 0, 2).reshape(8, width) + 128).astype(np.uint8))
        return np.ascontiguousarray(np.concatenate(rows, axis=0))


_sets = {}


def fixture_set(jpegamd, oracle, kind="full") -> FixtureSet:
    if kind not in _sets:
        _sets[kind] = FixtureSet(jpegamd, oracle, kind)
    return _sets[kind]


def verify(jpegamd, oracle, f):
    """Assert every claim of fixture `f` from the model (and from the grp_thr the library reports, which the model's constants hold)."""
    m = qm.evaluate(jpegamd, oracle, f.tile, f.table, f.quality)
    c = m.consts
    lanes_flagged = {32 * h + b for b in range(32) for h in (0, 1) if m.flags[b].reshape(4, 2, 8)[:, h].any()}
    flat = [b for b in range(32) if not f.tile[b].any()]
    assert all((m.hi_max[b, 1:] == 0).all() and not m.flags[b].any() for b in flat), f.name       # a flat block: no AC sum, no flag
    dead = qm.dead_groups(m).all(axis=0)                                  # per group: dead in every block, i.e. the tile skips it
    for what, arg in f.claims.items():
        if what == "live":
            G, h, b = arg
            coef = m.ref[b, 16 * G + 8 * h:16 * G + 8 * h + 8]
            assert sorted(np.abs(coef)) == [0] * 7 + [1], (f.name, coef)
            assert m.hi_max[b, G, h] >= c.grp_thr[G, h] and m.hi_max[b, G, 1 - h] < c.grp_thr[G, 1 - h], f.name
            assert len(flat) == 31 and not dead[G], f.name                # the group is alive through lane 32 h + b alone
            assert m.hi_max[b, G, h] < 1.5 * c.grp_thr[G, h], f.name      # ... and close to the edge
        elif what == "dead":
            G, b = arg
            assert len(flat) == 31 and f.tile[b].any() and dead[G], f.name
            assert (m.hi_max[b, G] < c.grp_thr[G]).all() and (m.hi_max[b, G] > 0).any(), f.name
            assert not m.ref[:, 16 * G:16 * G + 16].any() and not m.value[:, 16 * G:16 * G + 16].any(), f.name      # its zeros are right
        elif what == "upper_dead":
            assert (bool(dead[2]), bool(dead[3])) == arg, (f.name, dead)
        elif what == "nonzero_group":
            assert m.ref[:, 16 * arg:16 * arg + 16].any() and not dead[arg], f.name
        elif what == "lanes":
            assert lanes_flagged == set(arg), (f.name, sorted(lanes_flagged))
        elif what == "lane_sites":
            lane, nsites, ngroups = arg
            per_group = m.flags[lane & 31].reshape(4, 2, 8)[:, lane >> 5].sum(axis=1)
            assert lanes_flagged == {lane} and per_group.sum() == nsites, (f.name, per_group)
            assert ngroups is None or (per_group > 0).sum() == ngroups, (f.name, per_group)
        elif what == "flagged_groups":
            assert tuple(G for G in range(4) if m.flags[:, 16 * G:16 * G + 16].any()) == arg, f.name
        elif what == "own_half":
            G, h, b = arg
            fr = m.fract[:, 16 * G:16 * G + 16]
            assert c.flag_thr[G, h] > c.flag_thr[G, 1 - h] and m.flags[b].reshape(4, 2, 8)[G, h].any(), f.name
            assert fr.min() > np.float64(c.flag_thr[G, 1 - h]), f.name    # no lane of the tile passes the other half's threshold
        elif what == "differ":
            assert int((m.flags & (m.fast != m.ref)).sum()) >= arg, f.name
        elif what == "tie":
            assert int((m.flags & m.tie & (m.fast != m.ref)).sum()) >= arg, f.name
        else:
            raise AssertionError(f"unknown claim {what}")
    return m


def summary(jpegamd, oracle, kind="full"):
    """What the fixtures hold: their number, the quality each fallback fixture was found at, and per table the number of flagged sites
    and of those whose fast value is not the reference's, over the 256-wide planes."""
    s = fixture_set(jpegamd, oracle, kind)
    out = {"fixtures": len(s.fixtures), "quality": {f.name: f.quality for f in s.fixtures if f.quality != SKIP_QUALITY}}
    for table in ("luma", "chroma"):
        ms = [qm.plane_model(jpegamd, oracle, s.plane(q), table, q) for q in s.qualities()]
        out[table] = {"flagged": int(sum(m.flags.sum() for m in ms)), "differ": int(sum((m.flags & (m.fast != m.ref)).sum() for m in ms)),
                      "ties": int(sum((m.flags & m.tie & (m.fast != m.ref)).sum() for m in ms))}
    return out
