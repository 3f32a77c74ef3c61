"""Pictures that lie on the edges of the successive-approximation coder of DESIGN.md 4.6.14 -- TEST INFRASTRUCTURE ONLY, shared by
test_progressive_successive_host.py (which proves every edge on the model's counters) and test_gpu_progressive_successive.py.  Only
recipes: every picture is made here or cut from tests/golden/assets/lena.bmp."""
from __future__ import annotations

from pathlib import Path

import numpy as np

import color_model as cm
import progressive_runs_fixtures as rfx
import progressive_successive_model as psm

S444, S420, S422 = rfx.S444, rfx.S420, rfx.S422
SUBS = (S444, S420, S422)
FLAT, FLAT_513 = rfx.FLAT, rfx.FLAT_513                          # 8 x 8; 7 x 5 at 4:2:0 (pad blocks); 513 blocks: AC segments of 9 / 9 / 2 bits
CHAIN = (5464, 24, 90, S444)                                     # 2049 flat blocks: eight 9-bit segments at the bit phases 0 .. 7, then 2 bits
EDGE_Q = 95                                                      # progressive_runs_fixtures.edge_planes at this quality: the runs' edges with correction bits
NOISE_W, NOISE_H, NOISE_Q = 203, 117, 95                         # dense blocks: B and tails beyond 32 bits
REFINEMENT_SCANS = (6, 8, 9, 10)
LENA = Path(__file__).parent / "golden" / "assets" / "lena.bmp"


def flat_rgb(w, h, value):
    return rfx.flat_rgb(w, h, value)


def lena():
    from PIL import Image
    with Image.open(LENA) as f:
        return np.ascontiguousarray(np.asarray(f.convert("RGB")))


def lena_crop():
    """The 128 x 128 corner of the photograph: at quality 90 and 4:4:4 its refinement scans have ZRLs with pending correction bits and
    a block with two ZRLs."""
    return np.ascontiguousarray(lena()[:128, :128])


def noise_rgb():
    return np.random.default_rng(1).integers(0, 256, (NOISE_H, NOISE_W, 3), np.uint8)


def edge_planes():
    return rfx.edge_planes()


def edge_model(oracle):
    return cm.memo(psm.ycbcr_file, oracle, *edge_planes(), EDGE_Q, S444)


def synth_batch():
    """Three distinct 333 x 250 pictures: photo-like, noise, gradient."""
    return rfx.synth_batch()
