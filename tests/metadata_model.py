"""Metadata in front of the tables, restated in Python from the layout rule alone: the blob of marker segments, the 20
leading bytes with a pixel density, and the splice of both into a file written without them.  Shares no code with the library."""
from __future__ import annotations

PLAIN_HEAD = bytes.fromhex("ffd8ffe000104a46494600010101006000600000")
EXIF_MAX, PAYLOAD_MAX, ICC_CHUNK, ICC_CHUNKS_MAX, SEGMENTS_MAX = 65527, 65533, 65519, 255, 16
ICC_MAX = ICC_CHUNK * ICC_CHUNKS_MAX                                  # 16 707 345


def segment(marker: int, payload: bytes) -> bytes:
    if len(payload) > PAYLOAD_MAX:
        raise ValueError("a segment's payload is at most 65533 bytes")
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def blob(exif=None, segments=(), icc=None, comment=None) -> bytes:
    """Exif (the TIFF block, no identifier), the caller's segments [(marker, payload)], the ICC profile in chunks, the comment.
    None: no such segment; an empty Exif block or profile writes none either; an empty comment writes an empty COM segment."""
    out = b""
    if exif:
        if len(exif) > EXIF_MAX:
            raise ValueError("Exif above 65527 bytes")
        out += segment(0xE1, b"Exif\0\0" + exif)
    segments = list(segments)
    if len(segments) > SEGMENTS_MAX:
        raise ValueError("more than 16 segments")
    for marker, payload in segments:
        if not (0xE1 <= marker <= 0xEF or marker == 0xFE):
            raise ValueError(f"marker {marker:#x}")
        out += segment(marker, payload)
    if icc:
        if len(icc) > ICC_MAX:
            raise ValueError("an ICC profile of more than 255 chunks")
        chunks = [icc[i:i + ICC_CHUNK] for i in range(0, len(icc), ICC_CHUNK)]
        for k, chunk in enumerate(chunks):
            out += segment(0xE2, b"ICC_PROFILE\0" + bytes([k + 1, len(chunks)]) + chunk)
    if comment is not None:
        out += segment(0xFE, comment)
    return out


def head(density=None) -> bytes:
    """The 20 leading bytes: SOI and APP0, with density = (units, x, y) in bytes 13 .. 17, or 96 dpi."""
    if density is None:
        return PLAIN_HEAD
    units, x, y = density
    if units not in (0, 1, 2) or not 1 <= x <= 65535 or not 1 <= y <= 65535:
        raise ValueError("density")
    return PLAIN_HEAD[:13] + bytes([units]) + x.to_bytes(2, "big") + y.to_bytes(2, "big") + PLAIN_HEAD[18:]


def splice(file: bytes, head_bytes: bytes, blob_bytes: bytes) -> bytes:
    assert file[:20] == PLAIN_HEAD and len(head_bytes) == 20
    return head_bytes + blob_bytes + file[20:]


def icc_like(n: int, seed: int = 1) -> bytes:
    """n bytes that look like nothing in particular (an ICC profile is not interpreted by a JPEG writer), FF and 00 among them."""
    x, out = (seed * 2654435761 + 12345) & 0xFFFFFFFF, bytearray(n)
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x >> 24
    for i in range(7, n, 97):
        out[i] = 0xFF
    return bytes(out)
