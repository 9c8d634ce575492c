"""PNG files of 8-bit RGB images with the standard library alone (zlib, struct): what the preview entries write
(mosh_head.stageii_preview) and the tests read back.  Truecolour, 8 bits a channel, non-interlaced; no imaging library."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIGNATURE = b'\x89PNG\r\n\x1a\n'


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def _paeth(a, b, c):
    """The Paeth predictor of int arrays a (left), b (up), c (up-left)."""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def encode_png(rgb, filter_type=0, level=6):
    """The bytes of a PNG file for rgb[H, W, 3] uint8.  filter_type 0 .. 4 (none, sub, up, average, Paeth) is used on every row."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.shape[0] < 1 or rgb.shape[1] < 1:
        raise ValueError(f'write_png: the image must be uint8 [H, W, 3] with H, W >= 1, got {rgb.dtype} {tuple(rgb.shape)}')
    if filter_type not in (0, 1, 2, 3, 4):
        raise ValueError(f'write_png: filter_type must be 0 .. 4, got {filter_type!r}')
    H, W = rgb.shape[:2]
    raw = rgb.reshape(H, W * 3).astype(np.int32)
    left = np.zeros_like(raw); left[:, 3:] = raw[:, :-3]
    up = np.zeros_like(raw); up[1:] = raw[:-1]
    upleft = np.zeros_like(raw); upleft[1:, 3:] = raw[:-1, :-3]
    pred = (0, left, up, (left + up) // 2, _paeth(left, up, upleft))[filter_type]
    rows = np.empty((H, 1 + W * 3), dtype=np.uint8)
    rows[:, 0] = filter_type
    rows[:, 1:] = ((raw - pred) & 0xff).astype(np.uint8)
    ihdr = struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', zlib.compress(rows.tobytes(), level)) + _chunk(b'IEND', b'')


def write_png(fname, rgb, filter_type=0):
    """rgb[H, W, 3] uint8 -> an 8-bit truecolour, non-interlaced PNG file."""
    data = encode_png(rgb, filter_type)
    with open(fname, 'wb') as fh:
        fh.write(data)
    return fname


def decode_png(data):
    """rgb[H, W, 3] uint8 of the bytes of an 8-bit truecolour, non-interlaced PNG (row filters 0 .. 4); every chunk's CRC is checked."""
    if data[:8] != SIGNATURE:
        raise ValueError('read_png: not a PNG file (signature)')
    at, idat, head, ended = 8, [], None, False
    while at < len(data):
        if at + 12 > len(data):
            raise ValueError('read_png: truncated chunk')
        n, = struct.unpack('>I', data[at:at + 4])
        kind, body = data[at + 4:at + 8], data[at + 8:at + 8 + n]
        if len(body) != n or at + 12 + n > len(data):
            raise ValueError('read_png: truncated chunk')
        crc, = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
        if crc != (zlib.crc32(kind + body) & 0xffffffff):
            raise ValueError(f'read_png: bad CRC in chunk {kind!r}')
        at += 12 + n
        if kind == b'IHDR':
            head = struct.unpack('>IIBBBBB', body)
        elif kind == b'IDAT':
            idat.append(body)
        elif kind == b'IEND':
            ended = True
            break
    if head is None or not ended:
        raise ValueError('read_png: IHDR or IEND missing')
    W, H, depth, colour, comp, flt, interlace = head
    if (depth, colour, comp, flt, interlace) != (8, 2, 0, 0, 0):
        raise ValueError(f'read_png: only 8-bit truecolour, non-interlaced files are read, got depth {depth} colour {colour} interlace {interlace}')
    raw = zlib.decompress(b''.join(idat))
    stride = 1 + 3 * W
    if len(raw) != H * stride:
        raise ValueError(f'read_png: {len(raw)} bytes of image data, expected {H * stride}')
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, stride)
    out = np.zeros((H, 3 * W), dtype=np.int32)
    zero = np.zeros(3 * W, dtype=np.int32)
    for y in range(H):
        ft, line = int(rows[y, 0]), rows[y, 1:].astype(np.int32)
        prev = out[y - 1] if y else zero
        if ft == 0:
            out[y] = line
        elif ft == 2:
            out[y] = (line + prev) & 0xff
        elif ft == 1:   # each channel is a running sum along the row
            out[y] = (np.cumsum(line.reshape(W, 3), axis=0) & 0xff).reshape(-1)
        elif ft in (3, 4):
            cur = out[y]
            for x in range(3 * W):
                a = cur[x - 3] if x >= 3 else 0
                b = prev[x]
                if ft == 3:
                    p = (a + b) // 2
                else:
                    c = prev[x - 3] if x >= 3 else 0
                    pp = a + b - c
                    pa, pb, pc = abs(pp - a), abs(pp - b), abs(pp - c)
                    p = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[x] = (line[x] + p) & 0xff
        else:
            raise ValueError(f'read_png: row filter {ft} does not exist')
    return out.astype(np.uint8).reshape(H, W, 3)


def read_png(fname):
    with open(fname, 'rb') as fh:
        return decode_png(fh.read())
