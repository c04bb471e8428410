"""Hostile rate-state record headers and the verdict each must get in a slot of a given rate, worked by hand from the header's
documented order of checks (include/percepnet_hip.h: magic, version, the rate, then the size word).  One table for the host check
(tests/test_rate_pipe_host.py: pn_rate_state_check) and for the device import (tests/test_gpu_rate_pipe.py: d_status)."""
import struct

SS_OK, SS_BAD_MAGIC, SS_BAD_VERSION, SS_BAD_SIZE, SS_BAD_RATE = 0, -1, -2, -3, -6
STATE_BYTES = {8000: 912, 16000: 528, 24000: 400}          # 16 + 4 * (32 + 32 * 48000 / rate)
MAGIC = b"PNRS"


def header(magic=MAGIC, version=1, size=None, rate=8000):
    return struct.pack("<4sIIi", magic, version, STATE_BYTES[rate] if size is None else size, rate)


def hostile_headers(slot_rate):
    """-> [(name, 16 header bytes, verdict in a slot of slot_rate)]"""
    R = slot_rate
    other = 16000 if R == 8000 else 8000
    return [
        ("good", header(rate=R), SS_OK),
        ("magic", header(magic=b"PNRX", rate=R), SS_BAD_MAGIC),
        ("version", header(version=2, rate=R), SS_BAD_VERSION),
        ("other_rate", header(rate=other), SS_BAD_RATE),                                   # a whole, valid header of another rate
        ("size_word", header(size=STATE_BYTES[R] + 4, rate=R), SS_BAD_SIZE),
        ("magic_before_version", header(magic=b"\0\0\0\0", version=0, rate=R), SS_BAD_MAGIC),
        ("rate_before_size", struct.pack("<4sIIi", MAGIC, 1, STATE_BYTES[R], other), SS_BAD_RATE),
        ("unknown_rate", struct.pack("<4sIIi", MAGIC, 1, STATE_BYTES[R], 44100), SS_BAD_RATE),
        ("size_of_other_rate", struct.pack("<4sIIi", MAGIC, 1, STATE_BYTES[other], R), SS_BAD_SIZE),
    ]
