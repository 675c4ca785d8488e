"""A numpy model of csrc/rt_jpeg.h's decode of a baseline JPEG (DESIGN.md "JPEG on the device"): Huffman, jpeg_idct_islow, libjpeg's
"fancy" upsampling and its fixed-point YCbCr conversion.  Written from the formulas, held to PIL's decodes in tests/golden/jpeg_cases.npz
(test_jpeg_host.py); the library is then held to the same fixtures, never to this model.  `mutant` breaks one rule at a time, to show
that the fixtures tell: "no-round" drops the rounding of D, "duplicate" replaces the triangle filter by plain duplication, "plus8" makes
the 2x2 filter's +7 a +8."""
import struct

import numpy as np

ZZ = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
      57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class Refused(Exception):
    pass


def parse(d):
    if d[:2] != b"\xff\xd8":
        raise Refused("no SOI")
    i, q, h, sof, dri = 2, {}, {}, None, 0
    while True:
        if i + 4 > len(d) or d[i] != 0xFF:
            raise Refused("no marker")
        m = d[i + 1]
        L = struct.unpack(">H", d[i + 2:i + 4])[0]
        seg = d[i + 4:i + 2 + L]
        if i + 2 + L > len(d):
            raise Refused("segment past the end")
        if m == 0xDB:
            p = 0
            while p < len(seg):
                if seg[p] >> 4:
                    raise Refused("16-bit quantisers")
                q[seg[p] & 15] = list(seg[p + 1:p + 65])
                p += 65
        elif m == 0xC0:
            P, Y, X, N = struct.unpack(">BHHB", seg[:6])
            if N not in (1, 3):
                raise Refused("components")
            sof = (Y, X, [(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(N)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8):
            raise Refused("SOF%d" % (m - 0xC0))
        elif m == 0xC4:
            p = 0
            while p < len(seg):
                tc, th = seg[p] >> 4, seg[p] & 15
                bits = seg[p + 1:p + 17]
                vals = seg[p + 17:p + 17 + sum(bits)]
                p += 17 + sum(bits)
                code, k, tab = 0, 0, {}
                for ln in range(1, 17):
                    for _ in range(bits[ln - 1]):
                        tab[(ln, code)] = vals[k]
                        k += 1
                        code += 1
                    code <<= 1
                h[(tc, th)] = tab
        elif m == 0xDD:
            dri = struct.unpack(">H", seg[:2])[0]
        elif m == 0xDA:
            ns = seg[0]
            sc = [(seg[1 + 2 * k], seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15) for k in range(ns)]
            return q, h, sof, dri, sc, i + 2 + L
        i += 2 + L


def coefficients(d):
    q, h, (Y, X, comps), dri, sc, pos = parse(d)
    if len(comps) == 1:
        comps = [(comps[0][0], 1, 1, comps[0][3])]
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    mx, my = -(-X // (8 * hmax)), -(-Y // (8 * vmax))
    segs, cur, i = [], bytearray(), pos  # the clean stream, split at the restart markers
    while i < len(d):
        b = d[i]
        if b == 0xFF:
            n = d[i + 1] if i + 1 < len(d) else 0xD9
            if n == 0:
                cur.append(0xFF)
                i += 2
                continue
            if 0xD0 <= n <= 0xD7:
                segs.append(bytes(cur))
                cur = bytearray()
                i += 2
                continue
            break
        cur.append(b)
        i += 1
    segs.append(bytes(cur))
    coef = [np.zeros((my * c[2], mx * c[1], 64), np.int64) for c in comps]
    mcu = 0
    for s in segs:
        nb = len(s) * 8
        bs = (bin(int.from_bytes(s, "big"))[2:].zfill(nb) if nb else "")
        p = 0

        def hd(tab):
            nonlocal p
            code = 0
            for ln in range(1, 17):
                if p >= nb:
                    raise Refused("the stream ends early")
                code = (code << 1) | (bs[p] == "1")
                p += 1
                if (ln, code) in tab:
                    return tab[(ln, code)]
            raise Refused("a code that is not in its table")

        def recv(n):
            nonlocal p
            if n == 0:
                return 0
            if p + n > nb:
                raise Refused("the stream ends early")
            v = int(bs[p:p + n], 2)
            p += n
            return v if v >= (1 << (n - 1)) else v - (1 << n) + 1

        pred = [0] * len(comps)
        for _ in range(dri if dri else mx * my):
            if mcu >= mx * my:
                break
            my_, mx_ = divmod(mcu, mx)
            for ci, (cid, hh, vv, tq) in enumerate(comps):
                _, td, ta = sc[ci]
                for by in range(vv):
                    for bx in range(hh):
                        blk = coef[ci][my_ * vv + by, mx_ * hh + bx]
                        pred[ci] += recv(hd(h[(0, td)]))
                        blk[0] = pred[ci]
                        k = 1
                        while k < 64:
                            rs = hd(h[(1, ta)])
                            r, sz = rs >> 4, rs & 15
                            if sz == 0:
                                if r == 15:
                                    k += 16
                                    continue
                                break
                            k += r
                            if k > 63:
                                raise Refused("a coefficient index past 63")
                            blk[ZZ[k]] = recv(sz)
                            k += 1
            mcu += 1
        if nb - p >= 8 and dri and mcu < mx * my:
            raise Refused("blocks in front of a restart marker")
    if mcu != mx * my:
        raise Refused("the stream ends early")
    return q, (Y, X, comps), coef


def idct(c, qt, mutant=None):
    qn = np.zeros(64, np.int64)
    for k in range(64):
        qn[ZZ[k]] = qt[k]
    x = (c * qn).reshape(c.shape[:-1] + (8, 8))

    def pass_(v, sh):
        i0, i1, i2, i3, i4, i5, i6, i7 = v
        z1 = (i2 + i6) * 4433
        t2, t3 = z1 - i6 * 15137, z1 + i2 * 6270
        t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
        t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
        o0, o1, o2, o3 = i7, i5, i3, i1
        z1, z2, z3, z4 = o0 + o3, o1 + o2, o0 + o2, o1 + o3
        z5 = (z3 + z4) * 9633
        o0, o1, o2, o3 = o0 * 2446, o1 * 16819, o2 * 25172, o3 * 12299
        z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
        o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
        D = (lambda y: y >> sh) if mutant == "no-round" else (lambda y: (y + (1 << (sh - 1))) >> sh)
        return [D(t10 + o3), D(t11 + o2), D(t12 + o1), D(t13 + o0), D(t13 - o0), D(t12 - o1), D(t11 - o2), D(t10 - o3)]

    ws = np.stack(pass_([x[..., r, :] for r in range(8)], 11), axis=-2)
    out = np.stack(pass_([ws[..., :, col] for col in range(8)], 18), axis=-1)
    return np.clip(out + 128, 0, 255)


def up_h(p, mutant=None):
    if mutant == "duplicate":
        return np.repeat(p, 2, 1)
    prev, nxt = np.concatenate([p[:, :1], p[:, :-1]], 1), np.concatenate([p[:, 1:], p[:, -1:]], 1)
    o = np.zeros((p.shape[0], 2 * p.shape[1]), np.int64)
    o[:, 0::2], o[:, 1::2] = (3 * p + prev + 1) >> 2, (3 * p + nxt + 2) >> 2
    return o


def up_hv(p, mutant=None):
    if mutant == "duplicate":
        return np.repeat(np.repeat(p, 2, 0), 2, 1)
    up, dn = np.concatenate([p[:1], p[:-1]], 0), np.concatenate([p[1:], p[-1:]], 0)
    rows = np.zeros((2 * p.shape[0], p.shape[1]), np.int64)
    rows[0::2], rows[1::2] = 3 * p + up, 3 * p + dn
    prev, nxt = np.concatenate([rows[:, :1], rows[:, :-1]], 1), np.concatenate([rows[:, 1:], rows[:, -1:]], 1)
    o = np.zeros((rows.shape[0], 2 * rows.shape[1]), np.int64)
    o[:, 0::2], o[:, 1::2] = (rows * 3 + prev + 8) >> 4, (rows * 3 + nxt + (8 if mutant == "plus8" else 7)) >> 4
    return o


def to_rgb(d, mutant=None):
    """The bitmap [H, W, 3] uint8 of the JPEG bytes d; Refused for what the model does not decode."""
    q, (Y, X, comps), coef = coefficients(bytes(d))
    hmax, vmax = max(c[1] for c in comps), max(c[2] for c in comps)
    planes = []
    for ci, (cid, hh, vv, tq) in enumerate(comps):
        s = idct(coef[ci], q[tq], mutant)
        by, bx = s.shape[:2]
        p = s.transpose(0, 2, 1, 3).reshape(by * 8, bx * 8)[:-(-Y * vv // vmax), :-(-X * hh // hmax)]
        if (hh, vv) == (hmax, vmax):
            pass
        elif hmax == 2 * hh and vmax == vv:
            p = up_h(p, mutant)
        elif hmax == 2 * hh and vmax == 2 * vv:
            p = up_hv(p, mutant)
        else:
            raise Refused("sampling")
        planes.append(p[:Y, :X])
    if len(planes) == 1:
        return np.repeat(planes[0][..., None], 3, -1).astype(np.uint8)
    y, cb, cr = planes[0], planes[1] - 128, planes[2] - 128
    r, g, b = y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
