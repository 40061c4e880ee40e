"""numpy restatement of what csrc/wpack.h lays out for the kernels, written from the layouts the kernels document (the wfrag / w1 / w3 /
*frag comments of csrc/internal.h, the split pixel layout and the K-step rules there, conv_igemm_mfma's row order in kernels.hip) as
closed index formulas -- not from the packer's loops.  tests/test_wpack_cpu.py holds the header to it, bit for bit.

An MFMA A fragment is 64 lanes x 8 halves: lane l holds row (l & 15) of a 16-row block and the 8 consecutive K elements from
(l >> 4) * 8 of a 32-wide K slice.  `afrag` gives every fragment of a [cout][K] matrix at once; each form below is a reordering of it."""
import numpy as np

F16, BF16, F16X3, F32 = "f16", "bf16", "f16x3", "f32"
LANE = np.arange(64)
PAD_DY = 16000                      # a K-padding granule: a tap no source reaches


# ------------------------------------------------------------------------------------------------ inputs both sides generate
def lcg(n, seed):
    x = np.empty(n, np.uint32)
    v = seed & 0xFFFFFFFF
    for i in range(n):
        v = (v * 1664525 + 1013904223) & 0xFFFFFFFF
        x[i] = v
    return x


def weights(n, seed, variant):
    """fp32 weights in (-1, 1) on a 2^-15 grid; the variants exercise the pre-scale (zero / clamp / saturation / subnormal lo half)"""
    w = (((lcg(n, seed) >> 8) % 65535).astype(np.int64) - 32767).astype(np.float32) / np.float32(32768)
    if variant == "zero":
        w[:] = 0
    elif variant == "tiny":
        w = np.ldexp(w, -71).astype(np.float32)
        w[0] = np.ldexp(np.float32(1), -70)                    # max |w| = 2^-70: the exponent clamp (2^60)
    elif variant == "big":
        w[1] = 70000.0                                         # above the largest fp16
    else:
        w[2] = np.float32(300 + 2.0 ** -15) / np.float32(512)  # x 2^9: hi = 300, lo = 2^-15, a subnormal fp16
        w[3] = 0.75
    return w


def halves(n, seed):
    return ((lcg(n, seed) >> 8) & 0xFFFF).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ roundings
def f16_bits(v):
    return np.clip(np.asarray(v, np.float32), -65504, 65504).astype(np.float16).view(np.uint16)       # RNE, saturating


def bf16_bits(v):
    u = np.asarray(v, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def prescale(wmax):
    """the power of two that brings wmax into [256, 512), exponent held to +-60; 1 for wmax == 0"""
    if not wmax > 0:
        return np.float32(1)
    _, ex = np.frexp(np.float32(wmax))
    return np.float32(2.0 ** int(np.clip(9 - ex, -60, 60)))


def split_bits(v, wpre):
    sv = np.asarray(v, np.float32) * np.float32(wpre)
    hi = f16_bits(sv)
    lo = f16_bits(sv - hi.view(np.float16).astype(np.float32))
    return hi, lo


def wpre_of(precision, *ws):
    return prescale(max(float(np.abs(w).max()) for w in ws)) if precision == F16X3 else np.float32(1)


def planes(precision, v, wpre):
    """[1 or 2 planes] + v.shape: the 16-bit image of v (split mode: hi plane, lo plane)"""
    if precision == F16X3:
        return np.stack(split_bits(v, wpre))
    return (f16_bits(v) if precision == F16 else bf16_bits(v))[None]


# ------------------------------------------------------------------------------------------------ rows and fragments
def row_channel(row, cout):
    """output channel in packed weight row `row`: inside a wave tile of 64 channels (32 where the channel tile is 32, cout <= 32) MFMA row
    block mi, row rho holds channel (mi >> 1) * 32 + (rho >> 2) * 8 + (mi & 1) * 4 + (rho & 3) -- the epilogue's 16-byte NHWC stores"""
    row = np.asarray(row)
    wch = 32 if cout <= 32 else 64
    t = row % wch
    mi, rho = t >> 4, t & 15
    return row // wch * wch + (mi >> 1) * 32 + (rho >> 2) * 8 + (mi & 1) * 4 + (rho & 3)


def afrag(m, rows=None):
    """m: [R][K] -> [R / 16 row blocks][K / 32 slices][64 lanes][8]; rows: the matrix row each packed row holds (default: itself)"""
    R, K = m.shape
    r = np.arange(R // 16)[:, None] * 16 + (LANE & 15)                                              # [RB][64]
    r = r if rows is None else rows[r]
    k = np.arange(K // 32)[:, None, None] * 32 + (LANE >> 4)[None, :, None] * 8 + np.arange(8)      # [KS][64][8]
    return m[r[:, None, :, None], k[None]]


def wfrag(w_ck, cout):
    """fp32 [cout][K] -> fragments [K / 32][cout / 16][64][8], rows in row_channel order"""
    return afrag(w_ck, row_channel(np.arange(cout), cout)).transpose(1, 0, 2, 3)


# ------------------------------------------------------------------------------------------------ dedicated kernels
def stem(precision, w):
    """StemParams::wfrag [7 ky][4 mi][64][8] (split: that block twice, hi then lo).  w: [7][4 granules][8][64]"""
    f = wfrag(w.reshape(7 * 32, 64).T, 64)
    return planes(precision, f, wpre_of(precision, w)).ravel()


def direct64(precision, w):
    """Direct64Params::wfrag [9 taps][2 kk][4 mi][64][8] (split: twice).  w: [9][64 cin][64]"""
    f = wfrag(w.reshape(9 * 64, 64).T, 64)                    # K slice = tap * 2 + kk
    return planes(precision, f, wpre_of(precision, w)).ravel()


def block_w1(precision, w):
    """BlockParams::w1 [cin / 32 kk][4 mi][64][8]; split: [kk][mi][hi | lo][64][8].  w: [cin][64]"""
    p = planes(precision, wfrag(w.T, 64), wpre_of(precision, w))                  # [P][kk][mi][64][8]
    return p.transpose(1, 2, 0, 3, 4).ravel()


def block_w3(precision, wa, wb=None):
    """BlockParams::w3 [2 | 4 kk][16 mi][64][8], kk 0-1 contract wa, 2-3 wb; split: [kk][mi][hi | lo].  wa, wb: [64][256]"""
    w = wa if wb is None else np.concatenate([wa, wb])
    p = planes(precision, wfrag(w.T, 256), wpre_of(precision, w))
    return p.transpose(1, 2, 0, 3, 4).ravel()


def tail(precision, w0, wi):
    """TailParams::wfrag.  The tail is a 3x3 conv over [nearest-x2 upsampling of src0 (64 ch), image (3 ch)] -> 32: output row 2 i + py, tap
    ky reads upsampled row 2 i + py + ky - 1 = source row i + (py + ky - 1) // 2, so per parity the three taps fall on TWO source rows
    and the weights of taps on the same row are summed (fp32, ky then kx ascending).  K-steps 0-3 = source (row, column) pair
    (ks >> 1, ks & 1), k = channel; then the 9 image taps: plain modes one tap per 8-wide k-group over two K-steps, split mode two taps
    per k-group (4 channels each) in one.  Layout [4 parities][KS][2 kk][2 mi][64][8]; split: per parity [hi | lo][5][2][2][64][8].
    w0: [3][3][64][32], wi: [3][3][3][32]"""
    split = precision == F16X3
    KS = 5 if split else 6
    pre = np.zeros((4, KS, 64, 32), np.float32)
    for q in range(4):
        py, px = q >> 1, q & 1
        for ks in range(4):
            v = np.zeros((64, 32), np.float32)
            for ky in range(3):
                for kx in range(3):
                    if (py + ky - 1) // 2 - (py - 1) // 2 == ks >> 1 and (px + kx - 1) // 2 - (px - 1) // 2 == ks & 1:
                        v = v + w0[ky, kx]
            pre[q, ks] = v
        for t in range(9):
            if split:
                pre[q, 4, 4 * t:4 * t + 3] = wi[t // 3, t % 3]
            else:
                pre[q, 4 + t // 8, 8 * (t % 8):8 * (t % 8) + 3] = wi[t // 3, t % 3]
    f = np.stack([[wfrag(pre[q, ks].T, 32) for ks in range(KS)] for q in range(4)])                   # [q][ks][kk][mi][64][8]
    p = planes(precision, f, wpre_of(precision, pre))                                                   # [P][q][ks]...
    return p.transpose(1, 0, 2, 3, 4, 5, 6).ravel()


# ------------------------------------------------------------------------------------------------ re-laid packed matrices
def _pairs(mat):
    """[R][Ktot] halves -> [R / 16][Ktot / 64 K-steps][hi | lo][64][8]: a K-step is two 32-wide slices"""
    f = afrag(mat)
    return f.reshape(f.shape[0], f.shape[1] // 2, 2, 64, 8)


def dec_halo(mat, nsteps):
    """DecHaloParams::wfrag, one class: [K-steps][4 row blocks][hi | lo][64][8] of packed rows 0..63"""
    return _pairs(mat[:64])[:, :nsteps].transpose(1, 0, 2, 3, 4).ravel()


def conv3(mat, C, ks0):
    """C3ERParams::w2frag [K-steps][8 waves][C / 128 row blocks][hi | lo]: wave w owns row blocks w * C / 128 .."""
    return _pairs(mat[:C])[:, :ks0].transpose(1, 0, 2, 3, 4).ravel()              # row block = w * MI0 + m: already wave-major


def expand(mat, C, kch):
    """ExpRedParams::w3frag [4C / 256 chunks][C / kch K-steps][8 waves][2 row blocks][hi | lo]: chunk j = rows 256 j .., wave w 32 of them"""
    f = _pairs(mat[:4 * C])[:, :C // kch]                                         # [j * 16 + w * 2 + m][k]
    return f.reshape(C // 64, 8, 2, C // kch, 2, 64, 8).transpose(0, 3, 1, 2, 4, 5, 6).ravel()


def reduce(mat, C, kch):
    """ExpRedParams::w1frag [chunks j][256 / kch K-steps][8 waves][C / 128 row blocks][hi | lo]: chunk j contracts y channels 256 j .."""
    f = _pairs(mat[:C])[:, :4 * C // kch]                                         # [w * MI2 + m][j * G2S + k]
    return f.reshape(8, C // 128, C // 64, 256 // kch, 2, 64, 8).transpose(2, 3, 0, 1, 4, 5, 6).ravel()


# ------------------------------------------------------------------------------------------------ the generic conv
class Src:
    def __init__(self, C, channels, kh, kw, stride=1, pad=0, off=0):
        self.C, self.channels, self.kh, self.kw, self.stride, self.pad, self.off = C, channels, kh, kw, stride, pad, off


def conv_tables(precision, srcs):
    """conv_igemm_mfma's contraction order: source-major, then channel group (64 channels; 32 in the split mode), then tap, then the group's
    8-channel granules; a 3x3 stride-2 source walks its taps parity set by parity set; every source is padded to whole K-steps with
    granules no tap reaches.  A K-step has 8 slots: 8 granules, or in the split mode 4 granules' hi halves, then their lo halves.
    Returns (slots [(source | -1, ky, kx, first channel, part)], ktab [(dy, dx, coff)], ksteps [(dy, dx, coff, irregular)], per source)"""
    split, elem = precision == F16X3, 4 if precision == F32 else 2
    gps = 4 if split else 8
    slots, ktab, per_src = [], [], []
    for s, cs in enumerate(srcs):
        g8 = -(-cs.channels // 8)
        order = [0, 2, 6, 8, 1, 7, 3, 5, 4] if (cs.kh, cs.kw, cs.stride) == (3, 3, 2) else range(cs.kh * cs.kw)
        gran = [(s, t // cs.kw, t % cs.kw, g * 8) for cg in range(0, g8, gps) for t in order for g in range(cg, min(g8, cg + gps))]
        gran += [(-1, 0, 0, 0)] * (-len(gran) % gps)
        per_src.append(len(gran) // gps)
        G = min(cs.C, 32)                                      # split pixel: channel groups of G, each [G hi][G lo]
        for i in range(0, len(gran), gps):
            for part in range(2 if split else 1):
                for (ss, ky, kx, c0) in gran[i:i + gps]:
                    slots.append((ss, ky, kx, c0, part))
                    if ss < 0:
                        ktab.append((PAD_DY, 0, 0))
                    else:
                        half = (c0 // G * 2 * G + c0 % G + part * G) if split else c0
                        ktab.append((ky - cs.pad - cs.off, kx - cs.pad - cs.off, half * elem))
    ksteps = []
    for t in range(len(ktab) // 8):
        e, sl = ktab[8 * t:8 * t + 8], slots[8 * t:8 * t + 8]
        lo_off = min(srcs[sl[0][0]].C, 32) * elem
        regular = precision != F32 and all(x[0] == sl[0][0] for x in sl) and all(
            (dy, dx) == e[0][:2] and coff == e[0][2] + (16 * (g & 3) + (g >> 2) * lo_off if split else 16 * g) for g, (dy, dx, coff) in enumerate(e))
        ksteps.append(e[0] + (0 if regular else 1,))
    return slots, ktab, ksteps, per_src


def conv_meta(ksteps, per_src):
    lo, hi = [[127, 127], [127, 127]], [[-127, -127], [-127, -127]]
    for t, (dy, dx, _, _) in enumerate(ksteps):
        s = 0 if t < per_src[0] else 1
        lo[s], hi[s] = [min(lo[s][0], dy), min(lo[s][1], dx)], [max(hi[s][0], dy), max(hi[s][1], dx)]
    return (per_src + [0])[:2] + [len(ksteps)] + lo[0] + lo[1] + hi[0] + hi[1] + [int(not any(k[3] for k in ksteps))]


def conv_matrix(precision, srcs, cout, ws, slots):
    """[cout_pad][Ktot]: rows in row_channel order (fp32: as given), padded to the widest channel tile (256; fp32: 4); element (row, slot * 8 + q)
    = the slot's half of w[source][ky][kx][first channel + q][channel], 0 where the channel or the row does not exist"""
    pad_to = 4 if precision == F32 else 256
    cout_pad = -(-cout // pad_to) * pad_to
    rows = np.arange(cout_pad) if precision == F32 else row_channel(np.arange(cout_pad), cout)
    col = np.zeros((len(slots) * 8, cout), np.float32)
    part = np.zeros(len(slots) * 8, np.int64)
    for i, (s, ky, kx, c0, p) in enumerate(slots):
        if s >= 0:
            n = max(0, min(8, srcs[s].channels - c0))
            col[8 * i:8 * i + n] = ws[s][ky, kx, c0:c0 + n]
            part[8 * i:8 * i + 8] = p
    m = np.zeros((cout_pad, len(slots) * 8), np.float32)
    m[rows < cout] = col.T[rows[rows < cout]]
    if precision == F32:
        return m
    p = planes(precision, m, wpre_of(precision, *ws))
    return np.where(part[None] == 1, p[-1], p[0])
