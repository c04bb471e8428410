"""The numpy model of the rate converter's call-state record (include/percepnet_hip.h "call-state records"; the layout and the
verdict in C: percepnet_amd/csrc/pn_call_rules.h; the kernel: pn_rate_call.hip), imported as `from tests import call_state_model`.

pack() builds a record from the state the other models keep — plc_model.Plc (linear history, period, P, r, lost), agc_model.Agc and
lim_model.Lim (their four-word states) and the level array of mix_sel_model.mix — and unpack() writes one back into them; verdict()
restates pn_rate_call_state_check.  A record:

    header  4 words   magic | version | 10640 | section mask
    body    hist 1920 f32 (oldest first) | q 720 f32 | P r lost 0 | AGC lev gain adapted spare | LIM gain hold limited spare | level 0 0 0
"""
import numpy as np

F32, U32 = np.float32, np.uint32
MAGIC, VERSION, BYTES = 0x53434E50, 1, 10640
PLC, AGC, LIM, MIX = 1, 2, 4, 8
ALL = PLC | AGC | LIM | MIX
HEADER_WORDS = 4
W_HIST, W_Q, W_META, W_AGC, W_LIM, W_MIX, BODY_WORDS = 0, 1920, 2640, 2644, 2648, 2652, 2656
WORDS = HEADER_WORDS + BODY_WORDS
OK, BAD_MAGIC, BAD_VERSION, BAD_SIZE, BAD_ARG, BAD_STATE = 0, -1, -2, -3, -5, -7
P_MIN, P_MAX = 240, 720
SECTION = {PLC: (W_HIST, W_AGC), AGC: (W_AGC, W_LIM), LIM: (W_LIM, W_MIX), MIX: (W_MIX, BODY_WORDS)}   # body words [lo, hi) of a section


def empty(mask=0):
    """-> uint32 [WORDS]: a record whose sections are all zero"""
    w = np.zeros(WORDS, U32)
    w[:4] = (MAGIC, VERSION, BYTES, mask)
    return w


def pack(s, held, plc=None, agc=None, lim=None, levels=None):
    """The record of stream s as a converter holding `held` exports it -> uint8 [BYTES]"""
    w = empty(held)
    b = w[HEADER_WORDS:]
    if held & PLC:
        b[W_HIST:W_Q] = np.ascontiguousarray(plc.hist[s], dtype=F32).view(U32)
        b[W_Q:W_META] = np.ascontiguousarray(plc.q[s], dtype=F32).view(U32)
        b[W_META:W_META + 4] = (int(plc.P[s]), int(plc.r[s]), int(plc.lost[s]), 0)
    if held & AGC:
        b[W_AGC:W_AGC + 4] = np.frombuffer(agc.state[s].tobytes(), U32)
    if held & LIM:
        b[W_LIM:W_LIM + 4] = np.frombuffer(lim.state[s].tobytes(), U32)
    if held & MIX:
        b[W_MIX] = np.asarray(levels, F32).view(U32)[s]
    return w.view(np.uint8)


def unpack(record, s, held, plc=None, agc=None, lim=None, levels=None):
    """An ACCEPTED record into slot s of models of a converter holding `held`: present and held is written, held and absent is
    zeroed, present and not held is dropped"""
    w = np.frombuffer(np.ascontiguousarray(record).tobytes(), U32)
    assert w.size == WORDS
    present = int(w[3])
    b = w[HEADER_WORDS:]
    if held & PLC:
        plc.hist[s] = b[W_HIST:W_Q].view(F32)
        plc.q[s] = b[W_Q:W_META].view(F32)
        plc.P[s], plc.r[s], plc.lost[s] = int(b[W_META]), int(b[W_META + 1]), int(b[W_META + 2])
    if held & AGC:
        agc.state[s] = np.frombuffer(b[W_AGC:W_AGC + 4].tobytes(), agc.state.dtype)[0]
    if held & LIM:
        lim.state[s] = np.frombuffer(b[W_LIM:W_LIM + 4].tobytes(), lim.state.dtype)[0]
    if held & MIX:
        levels[s] = b[W_MIX:W_MIX + 1].view(F32)[0]
    return present


def verdict(record):
    """pn_rate_call_state_check restated: record is None, or anything bytes() takes"""
    if record is None:
        return BAD_ARG
    raw = np.ascontiguousarray(record).tobytes() if isinstance(record, np.ndarray) else bytes(record)
    if len(raw) < 16:
        return BAD_SIZE
    h = np.frombuffer(raw[:16], "<u4")
    if h[0] != MAGIC:
        return BAD_MAGIC
    if h[1] != VERSION:
        return BAD_VERSION
    if h[2] != BYTES or len(raw) != BYTES:
        return BAD_SIZE
    mask = int(h[3])
    if mask & ~ALL:
        return BAD_STATE
    b = np.frombuffer(raw[16:], "<u4")
    for bit, (lo, hi) in SECTION.items():
        if not mask & bit and b[lo:hi].any():
            return BAD_STATE
    f = b.view("<f4")
    with np.errstate(invalid="ignore"):
        if mask & PLC:
            P, r = int(b[W_META]), int(b[W_META + 1])
            if not (P == 0 or P_MIN <= P <= P_MAX) or (r > 0 and P == 0) or b[W_META + 3] != 0:
                return BAD_STATE
        if mask & AGC:
            lev, g = f[W_AGC], f[W_AGC + 1]
            if not lev >= 0 or (b[W_AGC + 1] != 0 and not (F32(1.0 / 1024.0) <= g <= F32(1024.0))) or b[W_AGC + 3] != 0:
                return BAD_STATE
        if mask & LIM:
            g = f[W_LIM]
            if (b[W_LIM] != 0 and not (g > 0 and g <= F32(1.0))) or b[W_LIM + 3] != 0:
                return BAD_STATE
        if mask & MIX:
            lv = f[W_MIX]
            if not (lv >= 0 and np.isfinite(lv)) or b[W_MIX + 1:W_MIX + 4].any():
                return BAD_STATE
    return OK
