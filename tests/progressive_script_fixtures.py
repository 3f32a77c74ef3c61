"""The scan scripts the progressive-script tests use -- TEST INFRASTRUCTURE ONLY, shared by
test_progressive_script_host.py (which proves what every script exercises on the model's counters) and test_gpu_progressive_script.py.
A scan is (components, Ss, Se, Ah, Al), components a tuple of indices: 0 Y, 1 Cb, 2 Cr."""
from __future__ import annotations

import numpy as np

import color_model as cm
import progressive_script_model as scm
import scan_model as sm
import progressive_successive_fixtures as sfx

S444, S420, S422 = sfx.S444, sfx.S420, sfx.S422
Y, CB, CR, ALL = (0,), (1,), (2,), (0, 1, 2)


def ac_all(ah=0, al=0, comps=(Y, CB, CR)):
    return [(c, 1, 63, ah, al) for c in comps]


# the built-in scripts: seven scans by spectral selection, libjpeg's jpeg_simple_progression for YCbCr and for one component
SPECTRAL = [(ALL, 0, 0, 0, 0), (Y, 1, 5, 0, 0), (CB, 1, 5, 0, 0), (CR, 1, 5, 0, 0), (Y, 6, 63, 0, 0), (CB, 6, 63, 0, 0), (CR, 6, 63, 0, 0)]
SUCCESSIVE = [(ALL, 0, 0, 0, 1), (Y, 1, 5, 0, 2), (CR, 1, 63, 0, 1), (CB, 1, 63, 0, 1), (Y, 6, 63, 0, 2), (Y, 1, 63, 2, 1), (ALL, 0, 0, 1, 0),
              (CR, 1, 63, 1, 0), (CB, 1, 63, 1, 0), (Y, 1, 63, 1, 0)]
GRAY_SUCCESSIVE = [(Y, 0, 0, 0, 1), (Y, 1, 5, 0, 2), (Y, 6, 63, 0, 2), (Y, 1, 63, 2, 1), (Y, 0, 0, 1, 0), (Y, 1, 63, 1, 0)]

# a mozjpeg-like split of the DC scan
SPLIT = [(Y, 0, 0, 0, 0), ((1, 2), 0, 0, 0, 0), (Y, 1, 8, 0, 2), (CB, 1, 8, 0, 0), (CR, 1, 8, 0, 0), (Y, 9, 63, 0, 2), (Y, 1, 63, 2, 1),
         (Y, 1, 63, 1, 0), (CB, 9, 63, 0, 0), (CR, 9, 63, 0, 0)]
# one-component DC with a point transform, its refinement, and a two-component DC refinement
DC_FORMS = [(Y, 0, 0, 0, 1), (CB, 0, 0, 0, 1), (CR, 0, 0, 0, 1), (Y, 0, 0, 1, 0), ((1, 2), 0, 0, 1, 0)] + ac_all()
# two tables in a two-component scan; Y pad blocks at 4:2:0
Y_CB = [((0, 1), 0, 0, 0, 0), (CR, 0, 0, 0, 0)] + ac_all()
DC_ONLY = [(ALL, 0, 0, 0, 0)]
# four refinement depths
DEEP = [(ALL, 0, 0, 0, 0), (Y, 1, 63, 0, 3), (Y, 1, 63, 3, 2), (Y, 1, 63, 2, 1), (Y, 1, 63, 1, 0)] + ac_all(comps=(CB, CR))
# single-coefficient bands; bands that start and end on and off a 16-byte group
EDGES = [(ALL, 0, 0, 0, 0)] + [(Y, a, b, 0, 0) for a, b in ((1, 1), (2, 7), (8, 8), (9, 62), (63, 63))] + ac_all(comps=(CB, CR))
# 16 scans and 16 tables exactly: two DC tables, fourteen AC scans, the DC refinement
LIMIT = ([(ALL, 0, 0, 0, 1)] + [(Y, a, b, 0, 0) for a, b in ((1, 2), (3, 5), (6, 9), (10, 14), (15, 20), (21, 27), (28, 35), (36, 63))] +
         [(c, a, b, 0, 0) for c in (CB, CR) for a, b in ((1, 5), (6, 20), (21, 63))] + [(ALL, 0, 0, 1, 0)])
GRAY_SPLIT = [(Y, 0, 0, 0, 0), (Y, 1, 5, 0, 0), (Y, 6, 63, 0, 0)]

COLOUR = {"SPLIT": SPLIT, "DC_FORMS": DC_FORMS, "Y_CB": Y_CB, "DC_ONLY": DC_ONLY, "DEEP": DEEP, "EDGES": EDGES, "LIMIT": LIMIT,
          "SPECTRAL": SPECTRAL, "SUCCESSIVE": SUCCESSIVE}
GRAYS = {"GRAY_SPLIT": GRAY_SPLIT, "GRAY_SUCCESSIVE": GRAY_SUCCESSIVE}
COMPLETE = ("SPLIT", "DC_FORMS", "Y_CB", "DEEP", "EDGES", "LIMIT")   # every coefficient of every component down to bit 0

FLAT = [(8, 8, 90), (7, 5, 200)]                                 # one block; one MCU with three pad blocks at 4:2:0
GRAY_257 = (2056, 8)                                             # 257 blocks: a DC refinement scan of one full segment and one of a single bit
SIZE_1344 = (333, 250)                                           # 4:2:0: 42 x 32 = 1344 Y blocks, five full segments and one of 64 blocks
CHAIN = sfx.CHAIN


def masks(script):
    """-> [(component bit mask, Ss, Se, Ah, Al)]: the scans as the C interface takes them."""
    return [(sum(1 << c for c in comps), ss, se, ah, al) for comps, ss, se, ah, al in script]


def libjpeg_text(script) -> str:
    """The script in the text form of libjpeg's -scans files."""
    return "".join(f"{','.join(map(str, comps))}: {ss}-{se}, {ah}, {al} ;\n" for comps, ss, se, ah, al in script)


def flat_rgb(w, h, value):
    return sfx.flat_rgb(w, h, value)


def crop_67x43():
    """9 x 6 blocks of the photograph: pad blocks at 4:2:0 and 4:2:2."""
    return np.ascontiguousarray(sfx.lena_crop()[:43, :67])


def gray_plane(w, h, seed=5):
    """A luma plane with photo-like content."""
    return np.ascontiguousarray(sm.luma_plane(cm.synth_rgb(w, h, seed, 0)))


def model(oracle, rgb, q, sub, script):
    return cm.memo(scm.rgb_file, oracle, rgb, q, sub, scm._key(script))


def gray_model(oracle, plane, q, script):
    return cm.memo(scm.gray_file, oracle, plane, q, scm._key(script))
