"""The numpy float32 model of the rate converter's in-band DTMF detector (include/percepnet_hip.h "DTMF detection"; the rule with its
roundings and its summation order: percepnet_amd/csrc/pn_dtmf_rules.h; kernel percepnet_amd/csrc/pn_rate_dtmf.hip).  Every operation
below is one float32 operation on float32 values — numpy never fuses a product into an add — and the 17 half sums run in the header's
order, so the host function (pn_dtmf_frame) and the kernel's states and reports are compared with it bit for bit.  It is vectorised
over streams: state [n, 24] uint32 words, rows [n, 480], report [n, 4] words.

The rule, for one frame of a stream with detection on, x its 480-sample row:
    tables     f = 697 770 852 941 | 1209 1336 1477 1633; m = (f[k] * j) % 48000, a = 6.283185307179586 * m / 48000.0 in float64,
               ct[k][j] = float32(cos a), st[k][j] = float32(sin a); the frame's rotation cr[k], ci[k] from m = (f[k] * 480) % 48000
    half sums  C[k] = sum x*ct[k], S[k] = sum x*st[k], Ec = sum x*x: products rounded separately; 120 groups of four summed from +0.0
               in index order; padded to 128; two halves of 64, each folded by the xor butterfly v[i] = v[i] + v[i ^ stride], stride
               32..1; the sum = half0[0] + half1[0]
    window     A = Cp + (C*cr - S*ci), B = Sp + (S*cr + C*ci), P[k] = A*A + B*B, E = Ep + Ec; then Cp, Sp, Ep = C, S, Ec
    peaks      Pr = -1, r = 0; k = 0..3: P[k] > Pr -> Pr = P[k], r = k; Pc, c likewise over k = 4..7
    hit        E <= FLT_MAX and E >= (min_rms*min_rms)*960 and Pr + Pc >= (purity*480)*E and Pc <= Pr*twist_fwd and Pr <= Pc*twist_rev
               and, for every other k of either group, P[k]*rel <= the group's peak
    d          ord("123A456B789C*0#D"[4 r + c]) on a hit, else 0
    debounce   1. d != 0 and d == cand: run += 1 (saturating at 65535); else cand = d, run = 1 if d else 0
               2. cur0 != 0 and d == cur0: gap = 0, dur += 1
               3. cur0 != 0 and d != cur0: gap += 1; gap >= off_frames: END, ended = cur0 with its dur, cur = gap = dur = 0; else dur += 1
               4. cur == 0 and d != 0 and run >= on_frames: cur = d, gap = 0, dur = run, count += 1, BEGIN, last4 = (last4 << 8) | d
    concealed  the state is untouched; report: ON | HELD_LOST | cur << 8, dur of cur, count, last4
    not on     state untouched, report row four zero words
Report: word 0 flags | cur << 8 | ended << 16; word 1 the dur of cur, or of the digit that just ended; word 2 count; word 3 last4."""
import numpy as np

F32 = np.float32
U32 = np.uint32
FRAME = 480
N_PARAMS = 7
MIN_RMS, PURITY, TWIST_FWD, TWIST_REV, REL, ON_FRAMES, OFF_FRAMES = range(7)
ON, HIT, BEGIN, END, HELD_LOST = 1, 2, 4, 8, 16
STATE_WORDS, REPORT_WORDS = 24, 4
FREQS = (697, 770, 852, 941, 1209, 1336, 1477, 1633)
DIGITS = "123A456B789C*0#D"
FLT_MAX = np.finfo(F32).max
DEFAULTS = np.array([0.005, 0.5, 6.3, 6.3, 6.3, 3.0, 2.0], F32)
RANGES = ((0.0, 1.0, False, False), (0.0, 1.0, True, False), (1.0, 100.0, False, False), (1.0, 100.0, False, False), (1.0, 100.0, False, False),
          (1.0, 100.0, False, True), (1.0, 100.0, False, True))          # (low, high, low end open, whole number) by parameter index
_XOR = {s: np.arange(64) ^ s for s in (32, 16, 8, 4, 2, 1)}
_CODES = np.array([ord(ch) for ch in DIGITS], U32)


def make_tables():
    """-> ct [8, 480], st [8, 480], rot [16] (cr then ci), float32, from float64 cos and sin"""
    f = np.array(FREQS, np.int64)[:, None]
    m = (f * np.arange(FRAME + 1, dtype=np.int64)[None, :]) % 48000
    a = 6.283185307179586 * m.astype(np.float64) / 48000.0
    c, s = np.cos(a).astype(F32), np.sin(a).astype(F32)
    return np.ascontiguousarray(c[:, :FRAME]), np.ascontiguousarray(s[:, :FRAME]), np.concatenate([c[:, FRAME], s[:, FRAME]])


CT, ST, ROT = make_tables()


def use_tables(ct, st, rot):
    """The model computes with these tables from now on (the library's, where numpy's cos or sin rounds an entry the other way)."""
    global CT, ST, ROT
    CT, ST, ROT = np.array(ct, F32).reshape(8, FRAME), np.array(st, F32).reshape(8, FRAME), np.array(rot, F32).reshape(16)


def params_ok(p):
    """-> the first bad index, or -1"""
    p = np.asarray(p, F32)
    for i, (lo, hi, open_lo, whole) in enumerate(RANGES):
        if not ((p[i] > F32(lo) if open_lo else p[i] >= F32(lo)) and p[i] <= F32(hi) and (not whole or p[i] == np.floor(p[i]))):
            return i
    return -1


def half_sums(rows):
    """rows [n, 480] -> float32 [n, 17]: C[0..7], S[0..7], Ec in the one order"""
    x = np.ascontiguousarray(rows, dtype=F32).reshape(-1, FRAME)
    n = x.shape[0]
    out = np.empty((n, 17), F32)
    with np.errstate(all="ignore"):
        for at in range(0, n, 256):
            xb = x[at:at + 256]
            w = np.concatenate([np.broadcast_to(CT[None], (xb.shape[0], 8, FRAME)), np.broadcast_to(ST[None], (xb.shape[0], 8, FRAME)), xb[:, None, :]], axis=1)
            p = (xb[:, None, :] * w).reshape(-1, 17, FRAME // 4, 4)
            g = np.zeros(p.shape[:3], F32)
            for i in range(4):
                g = g + p[..., i]
            v = np.zeros((xb.shape[0], 17, 128), F32)
            v[:, :, :FRAME // 4] = g
            h = v.reshape(-1, 17, 2, 64)
            for s in (32, 16, 8, 4, 2, 1):
                h = h + h[..., _XOR[s]]
            out[at:at + 256] = h[:, :, 0, 0] + h[:, :, 1, 0]
    return out


def _sat_inc(v):
    return np.where(v == U32(0xffffffff), v, v + U32(1)).astype(U32)


def step(params, state, sums, concealed=None):
    """The scalar rule over n streams with detection on.  state [n, 24] uint32 (not modified), sums [n, 17] -> (state', report [n, 4])"""
    prm = np.asarray(params, F32)
    st = np.array(state, U32).reshape(-1, STATE_WORDS)
    n = st.shape[0]
    sums = np.asarray(sums, F32).reshape(n, 17)
    lost = np.zeros(n, bool) if concealed is None else np.asarray(concealed, bool).reshape(n)
    cur0, gap0, dur0, count0, last40 = st[:, 18] & U32(0xff), st[:, 18] >> U32(16), st[:, 19], st[:, 20], st[:, 21]
    with np.errstate(all="ignore"):
        C, S, Ec = sums[:, :8], sums[:, 8:16], sums[:, 16]
        Cp, Sp, Ep = st[:, :8].view(F32), st[:, 8:16].view(F32), st[:, 16].view(F32)
        cr, ci = ROT[None, :8], ROT[None, 8:]
        A = Cp + (C * cr - S * ci)
        B = Sp + (S * cr + C * ci)
        P = A * A + B * B
        E = Ep + Ec
        Pr, Pc = np.full(n, -1.0, F32), np.full(n, -1.0, F32)
        r, c = np.zeros(n, np.int64), np.zeros(n, np.int64)
        for k in range(4):
            w = P[:, k] > Pr
            Pr, r = np.where(w, P[:, k], Pr), np.where(w, k, r)
            w = P[:, 4 + k] > Pc
            Pc, c = np.where(w, P[:, 4 + k], Pc), np.where(w, k, c)
        Emin = (prm[MIN_RMS] * prm[MIN_RMS]) * F32(960.0)
        need = (prm[PURITY] * F32(480.0)) * E
        hit = (E <= FLT_MAX) & (E >= Emin) & ((Pr + Pc) >= need) & (Pc <= Pr * prm[TWIST_FWD]) & (Pr <= Pc * prm[TWIST_REV])
        for k in range(4):
            hit &= ((r == k) | (P[:, k] * prm[REL] <= Pr)) & ((c == k) | (P[:, 4 + k] * prm[REL] <= Pc))
    d = np.where(hit, _CODES[4 * r + c], U32(0)).astype(U32)
    on_frames, off_frames = U32(int(prm[ON_FRAMES])), U32(int(prm[OFF_FRAMES]))
    cand0, run0 = st[:, 17] & U32(0xff), st[:, 17] >> U32(16)
    same = (d != 0) & (d == cand0)
    run = np.where(same, np.where(run0 == U32(0xffff), run0, run0 + U32(1)), np.where(d != 0, U32(1), U32(0))).astype(U32)
    cand = np.where(same, cand0, d).astype(U32)
    flags = np.where(hit, U32(ON | HIT), U32(ON)).astype(U32)
    live = cur0 != 0
    keep = live & (d == cur0)
    miss = live & (d != cur0)
    gap = np.where(keep, U32(0), np.where(miss, gap0 + U32(1), gap0)).astype(U32)
    end = miss & (gap >= off_frames)
    dur = np.where(end, U32(0), np.where(live, _sat_inc(dur0), dur0)).astype(U32)
    ended, ended_dur = np.where(end, cur0, U32(0)).astype(U32), np.where(end, dur0, U32(0)).astype(U32)
    cur = np.where(end, U32(0), cur0).astype(U32)
    gap = np.where(end, U32(0), gap).astype(U32)
    flags |= np.where(end, U32(END), U32(0)).astype(U32)
    begin = (cur == 0) & (d != 0) & (run >= on_frames)
    cur, gap, dur = np.where(begin, d, cur).astype(U32), np.where(begin, U32(0), gap).astype(U32), np.where(begin, run, dur).astype(U32)
    count = np.where(begin, _sat_inc(count0), count0).astype(U32)
    last4 = np.where(begin, (last40 << U32(8)) | d, last40).astype(U32)
    flags |= np.where(begin, U32(BEGIN), U32(0)).astype(U32)
    new = np.zeros_like(st)
    new[:, :8], new[:, 8:16], new[:, 16] = C.view(U32), S.view(U32), np.ascontiguousarray(Ec).view(U32)
    new[:, 17], new[:, 18], new[:, 19], new[:, 20], new[:, 21] = cand | (run << U32(16)), cur | (gap << U32(16)), dur, count, last4
    rep = np.stack([flags | (cur << U32(8)) | (ended << U32(16)), np.where(cur != 0, dur, ended_dur), count, last4], axis=1).astype(U32)
    held = np.stack([U32(ON | HELD_LOST) | (cur0 << U32(8)), np.where(cur0 != 0, dur0, U32(0)), count0, last40], axis=1).astype(U32)
    new[lost] = st[lost]
    rep[lost] = held[lost]
    return new, rep


def frame(params, state, rows, on=None, concealed=None):
    """One frame of n streams.  state [n, 24] uint32, rows [n, 480]; on [n] (None: everybody), concealed [n] (None: nobody)
    -> (state', report [n, 4]); a stream that is not on keeps its state and reports four zero words"""
    st = np.array(state, U32).reshape(-1, STATE_WORDS)
    n = st.shape[0]
    x = np.asarray(rows, F32).reshape(n, FRAME)
    lost = np.zeros(n, bool) if concealed is None else np.asarray(concealed, bool).reshape(n)
    # a concealed stream's row is not read: its sums do not enter the rule
    new, rep = step(params, st, half_sums(np.where(lost[:, None], F32(0.0), x)), lost)
    if on is not None:
        off = ~np.asarray(on, bool).reshape(n)
        new[off] = st[off]
        rep[off] = 0
    return new, rep


def fresh(n):
    return np.zeros((n, STATE_WORDS), U32)


def digits_begun(reports):
    """reports [frames, 4] of ONE stream -> the digits whose BEGIN the frames carry, as a string"""
    rep = np.asarray(reports, U32).reshape(-1, REPORT_WORDS)
    return "".join(chr(int((w >> 8) & 0xff)) for w in rep[:, 0] if int(w) & BEGIN)


def dual_tone(digit, n, amp_row=0.1, amp_col=None, start=0, df_row=0.0, df_col=0.0):
    """n samples at 48 kHz of the digit's two sines from phase 0, float64; df_*: relative frequency offsets"""
    i = DIGITS.index(digit)
    fr, fc = FREQS[i // 4] * (1.0 + df_row), FREQS[4 + i % 4] * (1.0 + df_col)
    t = (np.arange(n) + start) / 48000.0
    return amp_row * np.sin(2 * np.pi * fr * t) + (amp_row if amp_col is None else amp_col) * np.sin(2 * np.pi * fc * t)


def keypad(digits=DIGITS, on=1920, off=1920, lead=0, amp=0.1, tail=1920):
    """The digits one after the other, `on` samples of tone and `off` of silence each, behind `lead` samples of silence; padded with
    silence to whole frames -> float32 [frames, 480]"""
    parts = [np.zeros(lead)]
    for ch in digits:
        parts += [dual_tone(ch, on, amp), np.zeros(off)]
    parts.append(np.zeros(tail))
    x = np.concatenate(parts)
    x = np.concatenate([x, np.zeros((-x.size) % FRAME)])
    return x.astype(F32).reshape(-1, FRAME)


def run_stream(params, rows, concealed=None):
    """One stream over rows [frames, 480] from the fresh state -> (reports [frames, 4], final state [24])"""
    rows = np.asarray(rows, F32).reshape(-1, FRAME)
    sums = half_sums(rows)
    st = fresh(1)
    reps = np.empty((rows.shape[0], REPORT_WORDS), U32)
    for i in range(rows.shape[0]):
        lost = None if concealed is None else np.array([bool(concealed[i])])
        st, rep = step(params, st, sums[i:i + 1], lost)
        reps[i] = rep[0]
    return reps, st[0]
