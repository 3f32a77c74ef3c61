"""What the GPU suites (tests/test_gpu_*.py) share -- TEST INFRASTRUCTURE ONLY: the device fixture, the sentinels of the C header, pictures
and planes, rows stored at a stride, guarded output buffers, and the batches queued on a context.  The files "by definition" come from
the model modules (color_model.py, color_model_422.py) through color_model.memo, one cache for every suite."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import scan_model as sm
from color_model import CBCR, CRCB, PLANES
from threshold_fixtures import gray_bmp                         # noqa: F401  (the bare-header BMP with R = G = B, either row order)

torch = pytest.importorskip("torch")

S444, S420, S422, GRAY = cm.SUB_444, cm.SUB_420, m422.SUB_422, 0
YUYV, UYVY = m422.YUYV, m422.UYVY
LAYOUTS = (PLANES, CBCR, CRCB)                                 # what every subsampling takes; 4:2:2 also takes the packed two
LAYOUTS_422 = LAYOUTS + (YUYV, UYVY)
WIDE_STRIDE = (1 << 24) + 64
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("gpu-marked test started without a GPU: the product path has no CPU fallback")
    return torch.device("cuda:0")


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- pictures and planes ------------------------------------------------------------------------------------------------------------
def gray_bmp_sized(p: np.ndarray) -> bytes:
    """The bottom-up BMP whose pixels are (p, p, p), its luma p itself ((77 + 150 + 29) p >> 8), as color_model.write_bmp writes it: the
    pixels of gray_bmp(p), and a header that also carries the image size and a resolution."""
    return cm.write_bmp(np.repeat(p[:, :, None], 3, axis=2))


def synth_rgb(jpegamd, w, h, seed, kind, flags=0):
    return cm.synth_rgb(w, h, seed, kind, flags)


def pictures(jpegamd, w, h, n, seed=0, base=100, step=37):
    """n distinct pictures: photo-like, noise, photo-like, gradient and flat content in turn, seeds base + step i + seed."""
    kinds = (0, 1, 0, 3, 2)
    return [synth_rgb(jpegamd, w, h, base + step * i + seed, kinds[i % len(kinds)], i % 4) for i in range(n)]


def rows_for(count, h):
    """The context height a batch of `count` pictures of h rows needs: count x the block rows of one picture."""
    return count * ((h + 7) // 8 * 8)


def chroma_dims(w, h, sub):
    return (w if sub == S444 else (w + 1) // 2), ((h + 1) // 2 if sub == S420 else h)


def random_planes(w, h, sub, seed):
    """(y, cb, cr) of uniform noise: uint8 [H, W], [ch, cw], [ch, cw]."""
    rng = np.random.default_rng(seed)
    cw, ch = chroma_dims(w, h, sub)
    return rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 256, (ch, cw), np.uint8), rng.integers(0, 256, (ch, cw), np.uint8)


def smooth_planes(w, h, sub, seed):
    """(y, cb, cr) of photo-like content: the model's planes of a synthetic picture (small files)."""
    import jpegamd
    return sm.planes_of(synth_rgb(jpegamd, w, h, seed, 0), sub)


def block_rows_reversed(plane):
    """The same tiles in the opposite order (another picture of the same geometry for a batch)."""
    h, w = plane.shape
    return np.ascontiguousarray(plane.reshape(h // 8, 8, w)[::-1].reshape(h, w))


def model(oracle, rgb, quality, sub):
    """The file the packed RGB path must write for these pixels: colour at `sub`, or (GRAY) the oracle's grayscale file."""
    if sub == S422:
        return cm.memo(m422.color_file_422, oracle, cm.write_bmp(rgb), quality)
    return cm.memo(cm.rgb_file, oracle, rgb, quality, sub)


def ycc_file(oracle, planes, quality, sub):
    """The file by definition of samples that already are Y, Cb and Cr."""
    if sub == S422:
        return cm.memo(m422.ycbcr_file_422, oracle, *planes, quality)
    return cm.memo(cm.ycbcr_file, oracle, *planes, quality, sub)


# ---- sources on the device ----------------------------------------------------------------------------------------------------------
def stored_rows(arr: np.ndarray, bottom_up: bool, bgr: bool = False) -> np.ndarray:
    """uint8 [H, W] (GRAY) or [H, W, 3] (R, G, B) -> the rows as the API reads them: [H, row bytes], first stored row first."""
    s = arr[::-1] if bottom_up else arr
    if bgr:
        s = s[:, :, ::-1]
    return np.ascontiguousarray(s).reshape(s.shape[0], -1)


def as_bytes(plane) -> np.ndarray:
    """[H, W] samples of one or two bytes -> [H, bytes] as they lie in memory (16-bit words little-endian)."""
    p = np.ascontiguousarray(plane)
    if p.dtype.itemsize == 2:
        p = p.astype("<u2")
    return p.view(np.uint8).reshape(p.shape[0], -1)


def upload(rows: np.ndarray, dev, stride: int, shift: int = 0):
    """[H, n] bytes ([H, W, 3]: n = 3 W) as H rows `stride` bytes apart, the first at byte `shift` of a zero-filled allocation that ends 16
    bytes behind the last row -> (tensor, device pointer of the first row)."""
    rows = rows.reshape(rows.shape[0], -1)
    h, n = rows.shape
    t = torch.zeros(shift + stride * (h - 1) + n + 16, dtype=torch.uint8, device=dev)
    t[shift:shift + stride * (h - 1) + n].as_strided((h, n), (stride, 1)).copy_(torch.from_numpy(rows.copy()).to(dev))
    return t, t.data_ptr() + shift


def upload_pixels(bmp: bytes, jpegamd, dev):
    """The pixel rows of a BMP file as they lie in it -> (its parsed header, tensor)."""
    img, off = jpegamd.parse_bmp(bmp)
    n = img.row_stride * img.height
    return img, torch.frombuffer(bytearray(bmp[off:off + n]), dtype=torch.uint8).to(dev)


# ---- guarded outputs ----------------------------------------------------------------------------------------------------------------
class Outputs:
    """n output buffers of `cap` bytes, each `out_off` bytes into its allocation with GUARD bytes behind it, everything filled with FILL;
    and their device sizes, preset to -1."""

    def __init__(self, dev, n, cap, out_off=0):
        self.cap, self.off = cap, out_off
        self.outs = [torch.full((out_off + cap + GUARD,), FILL, dtype=torch.uint8, device=dev) for _ in range(n)]
        self.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self.out_ptrs = [o.data_ptr() + out_off for o in self.outs]
        self.size_ptrs = [self.sizes.data_ptr() + 8 * i for i in range(n)]

    def results(self):
        """-> [(file bytes, guards intact)] picture by picture: the bytes behind the capacity, and those in front of the output, still
        hold FILL.  A file is cut at the capacity; a size that was never written reads as the whole capacity."""
        res = []
        for o, n in zip(self.outs, self.sizes.cpu().tolist()):
            host = o.cpu().numpy()
            intact = bool(np.all(host[self.off + self.cap:] == FILL) and np.all(host[:self.off] == FILL))
            res.append((bytes(host[self.off:self.off + (min(n, self.cap) if n >= 0 else self.cap)]), intact))
        return res


def intact_files(outputs):
    res = outputs.results()
    assert all(ok for _, ok in res), "guard bytes around an output were overwritten"
    return [f for f, _ in res]


def finish_files(enc, outputs):
    """Finish what is queued on `enc`: every guard intact, Stats.jfif_bytes the size of the last file -> (files, Stats)."""
    st = enc.finish()
    files = intact_files(outputs)
    assert st.jfif_bytes == len(files[-1])
    return files, st


# ---- calls queued on a context (not finished) -----------------------------------------------------------------------------------------
class ColorCall(Outputs):
    """One colour call (jpegamd_encode_color_async): the pixels stored as asked, the output `out_off` bytes past a 256-byte boundary."""

    def __init__(self, jpegamd, enc, rgb, dev, sub, quality=0, bgr=False, bottom_up=False, stride=None, shift=0, cap=None, out_off=0):
        h, w, _ = rgb.shape
        self.stride = stride or 3 * w
        self.px, ptr = upload(stored_rows(rgb, bottom_up, bgr), dev, self.stride, shift)
        super().__init__(dev, 1, cap if cap is not None else jpegamd.max_jfif_bytes_color(w, h, sub), out_off)
        self.size = self.sizes
        img = jpegamd.Encoder.image(ptr, w, h, self.stride, bottom_up, jpegamd.ORDER_BGR if bgr else jpegamd.ORDER_RGB, quality)
        enc.encode_color_async(img, sub, self.out_ptrs[0], self.cap, self.size_ptrs[0], stream())

    def result(self):
        return self.results()[0]


class ColorBatch(Outputs):
    """One colour batch (jpegamd_encode_color_batch_async): every picture stored as asked (shifts: per picture)."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, quality=0, bgr=False, bottom_up=False, stride=None, shifts=None, cap=None):
        h, w, _ = rgbs[0].shape
        self.stride = stride or 3 * w
        shifts = shifts or [0] * len(rgbs)
        self.px = [upload(stored_rows(r, bottom_up, bgr), dev, self.stride, s) for r, s in zip(rgbs, shifts)]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_color(w, h, sub))
        order = jpegamd.ORDER_BGR if bgr else jpegamd.ORDER_RGB
        imgs = [jpegamd.Encoder.image(ptr, w, h, self.stride, bottom_up, order, quality) for _, ptr in self.px]
        enc.encode_color_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, stream())


class YccBatch(Outputs):
    """One YCbCr batch.  Every stored plane lies `shift` bytes into its allocation with rows `stride` BYTES apart (y_*: the Y plane, or the
    packed plane of YUYV / UYVY; c_*: the chroma planes or the pair plane; shifts per picture).  sample_format: None for bytes, or
    jpegamd.SAMPLES_10_MSB / _LSB for uint16 planes.  entry: "encoder" goes through Encoder.encode_ycbcr_batch_async, which gets
    sample_range / sample_format only where they are given; "range" and "samples" call jpegamd_encode_ycbcr_range_batch_async and
    jpegamd_encode_ycbcr_samples_batch_async (SAMPLES_8 unless given) themselves, whatever entry Encoder would take."""

    def __init__(self, jpegamd, enc, planes, dev, sub, layout, quality=0, y_stride=None, c_stride=None, y_shifts=None, c_shifts=None,
                 cap=None, sample_range=None, sample_format=None, entry="encoder"):
        h, w = planes[0][0].shape
        cw, ch = chroma_dims(w, h, sub)
        n = len(planes)
        wide = sample_format is not None and sample_format != jpegamd.SAMPLES_8
        packed = layout in (YUYV, UYVY)
        assert not (packed and wide)
        self.y_stride = y_stride or (4 * cw if packed else w) * (2 if wide else 1)
        self.c_stride = c_stride or (cw if layout == PLANES else 2 * cw) * (2 if wide else 1)
        y_shifts, c_shifts = y_shifts or [0] * n, c_shifts or [0] * n
        self.keep, imgs = [], []
        for (y, cb, cr), ys, cs in zip(planes, y_shifts, c_shifts):
            assert cb.shape == (ch, cw) and cr.shape == (ch, cw)
            assert not wide or y.dtype == cb.dtype == cr.dtype == np.uint16
            if packed:
                t, p = upload(m422.pack_yuyv(y, cb, cr, "yuyv" if layout == YUYV else "uyvy"), dev, self.y_stride, ys)
                self.keep.append(t)
                imgs.append(jpegamd.Encoder.ycbcr_image(p, 0, 0, w, h, self.y_stride, 0, layout, quality))
                continue
            ty, py = upload(as_bytes(y), dev, self.y_stride, ys)
            # (chroma_rows interleaves sample by sample: 16-bit words stay whole)
            ups = [upload(as_bytes(rows), dev, self.c_stride, cs) for rows in cm.chroma_rows(cb, cr, layout)]
            self.keep.append((ty, ups))
            imgs.append(jpegamd.Encoder.ycbcr_image(py, ups[0][1], ups[1][1] if layout == PLANES else 0, w, h, self.y_stride,
                                                    self.c_stride, layout, quality))
        super().__init__(dev, n, cap if cap is not None else jpegamd.max_jfif_bytes_color(w, h, sub))
        if entry == "encoder":
            kw = {k: v for k, v in (("sample_range", sample_range), ("sample_format", sample_format)) if v is not None}
            enc.encode_ycbcr_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, stream(), **kw)
            return
        arr = (jpegamd.YCbCrImage * n)(*imgs)
        outs = (C.c_void_p * n)(*[C.c_void_p(p) for p in self.out_ptrs])
        sizes = (C.c_void_p * n)(*[C.c_void_p(p) for p in self.size_ptrs])
        if entry == "range":
            rc = jpegamd.lib.jpegamd_encode_ycbcr_range_batch_async(enc._h, arr, n, int(sub), int(sample_range), outs, self.cap, sizes,
                                                                    C.c_void_p(stream()))
        else:
            assert entry == "samples"
            fmt = jpegamd.SAMPLES_8 if sample_format is None else sample_format
            rc = jpegamd.lib.jpegamd_encode_ycbcr_samples_batch_async(enc._h, arr, n, int(sub), int(sample_range), fmt, outs, self.cap,
                                                                      sizes, C.c_void_p(stream()))
        assert rc == 0, rc


def run_ycc(jpegamd, enc, planes, dev, sub, layout, **kw):
    return finish_files(enc, YccBatch(jpegamd, enc, planes, dev, sub, layout, **kw))[0]


# ---- grayscale encodes with plain outputs ---------------------------------------------------------------------------------------------
def _plain_outputs(dev, n, cap):
    return [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)], [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(n)]


def encode_gray(jpegamd, enc, p, dev, bottom_up=False, stride=None, shift=0, quality=0):
    """One GRAY plane through jpegamd_encode_async -> the file; its size is Stats.jfif_bytes."""
    h, w = p.shape
    t, ptr = upload(stored_rows(p, bottom_up), dev, stride or w, shift)
    cap = jpegamd.max_jfif_bytes(w, h)
    (out,), (size,) = _plain_outputs(dev, 1, cap)
    enc.encode_async(jpegamd.Encoder.image(ptr, w, h, stride or w, bottom_up, jpegamd.ORDER_GRAY, quality), out.data_ptr(), cap,
                     size.data_ptr(), True, stream())
    st = enc.finish()
    n = int(size.item())
    assert n == st.jfif_bytes
    return bytes(out[:n].cpu().numpy())


def encode_gray_planes(jpegamd, enc, planes, dev, q):
    """GRAY planes of one geometry: one call of jpegamd_encode_async, or one batch -> (files, Stats)."""
    h, w = planes[0].shape
    keep = [upload(p, dev, w) for p in planes]
    cap = jpegamd.max_jfif_bytes(w, h)
    outs, sizes = _plain_outputs(dev, len(planes), cap)
    imgs = [jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, q) for _, ptr in keep]
    if len(planes) == 1:
        enc.encode_async(imgs[0], outs[0].data_ptr(), cap, sizes[0].data_ptr(), True, stream())
    else:
        enc.encode_batch_async(imgs, [o.data_ptr() for o in outs], cap, [s.data_ptr() for s in sizes], True, stream())
    st = enc.finish()
    return [bytes(o[:int(s.item())].cpu().numpy()) for o, s in zip(outs, sizes)], st


def device_encode(jpegamd, enc, bmp, dev, quality=0, container=True, cap=None):
    """The pixels of a BMP file (BGR, its own stride and row order) through jpegamd_encode_async -> (file or segment, Stats)."""
    img, px = upload_pixels(bmp, jpegamd, dev)
    cap = cap or (4096 + 2 * img.width * img.height)
    (out,), (size,) = _plain_outputs(dev, 1, cap)
    d = jpegamd.Encoder.image(px.data_ptr(), img.width, img.height, img.row_stride, bool(img.bottom_up), jpegamd.ORDER_BGR, quality)
    enc.encode_async(d, out.data_ptr(), cap, size.data_ptr(), container, stream())
    st = enc.finish()
    n = int(size.item())
    assert n == st.jfif_bytes
    return bytes(out[:n].cpu().numpy()), st
