"""The numpy model of the G.711 companding at the rate converter's 8-bit edges (include/percepnet_hip.h "G.711 streams";
percepnet_amd/csrc/pn_g711.h): integer formulas with one answer per input, written from the header's text and independent of the
library.  decode: uint8 -> int16; encode: int16 -> uint8; every intermediate value is int32."""
import numpy as np

ULAW, ALAW = 0, 1
LAWS = (ULAW, ALAW)
NAMES = {ULAW: "ulaw", ALAW: "alaw"}
SILENCE = {ULAW: 0xFF, ALAW: 0xD5}
# known answers (all 256 codes and all 65 536 values were run through the formulas)
ENC_KNOWN = {ULAW: {0: 0xFF, -1: 0x7F, 32767: 0x80, -32768: 0x00, -4: 0x7F, -5: 0x7E},
             ALAW: {0: 0xD5, -1: 0x55, 32767: 0xAA, -32768: 0x2A}}
DEC_RANGE = {ULAW: 32124, ALAW: 32256}
MAX_ROUND_TRIP_ERROR = {ULAW: 644, ALAW: 512}


def _floor_log2(x):
    """floor(log2 x) of positive int32 values, by comparison with the powers of two (no floating point)"""
    out = np.zeros(x.shape, np.int32)
    for k in range(1, 16):
        out += (x >= (1 << k)).astype(np.int32)
    return out


def decode(law, b):
    b = np.asarray(b).astype(np.int32) & 0xFF
    if law == ULAW:
        u = ~b & 0xFF
        e, m = (u >> 4) & 7, u & 15
        mag = (((m << 3) + 132) << e) - 132
        v = np.where(u & 0x80, -mag, mag)
    elif law == ALAW:
        a = b ^ 0x55
        e, m = (a >> 4) & 7, a & 15
        mag = np.where(e == 0, (m << 4) + 8, ((m << 4) + 264) << np.maximum(e - 1, 0))
        v = np.where(a & 0x80, mag, -mag)
    else:
        raise ValueError(law)
    return v.astype(np.int16)


def encode(law, v):
    v = np.asarray(v).astype(np.int32)
    assert v.min(initial=0) >= -32768 and v.max(initial=0) <= 32767
    neg = v < 0
    mag = np.where(neg, ~v, v)
    if law == ULAW:
        p = np.minimum((mag >> 2) + 33, 8191)
        e = _floor_log2(p) - 5
        m = (p >> (e + 1)) & 15
        b = ~(np.where(neg, 0x80, 0) | (e << 4) | m) & 0xFF
    elif law == ALAW:
        e = np.where(mag < 256, 0, _floor_log2(np.maximum(mag, 1)) - 7)
        m = np.where(e == 0, mag >> 4, mag >> (e + 3)) & 15
        b = (np.where(neg, 0, 0x80) | (e << 4) | m) ^ 0x55
    else:
        raise ValueError(law)
    return b.astype(np.uint8)


def decode_rows(laws, b):
    """b uint8 [B, n] with the law of row s in laws[s] -> int16 [B, n]"""
    return np.stack([decode(int(w), row) for w, row in zip(laws, b)])


def encode_rows(laws, v):
    return np.stack([encode(int(w), row) for w, row in zip(laws, v)])
