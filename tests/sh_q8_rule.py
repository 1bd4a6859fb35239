"""The value contract of MSPLAT_STORAGE_SH_Q8 (include/msplat.h) restated in numpy, and the hand-made records
both SH_Q8 test files use.  Inputs and the rule only: nothing here calls the library.

Per splat and SH band (band 1: 9 values, band 2: 15, band 3: 21; r, g and b together), all in fp32:
    m = max |c|;  m < 2^-64: step = 0, codes 0;  else step = m / 127, code = clamp(rint(c / step), -127, 127), halves to even;
    stored value c' = (float)code * step."""
import numpy as np

# f_rest columns of the reference record (61 floats: pos+alpha, r/g/b_sh0 = DC + band 1, Sigma, r/g/b_sh1..3 = bands 2-3)
REST = [5, 6, 7, 9, 10, 11, 13, 14, 15] + list(range(25, 61))
# SH band (0..2) of REST[h]: the first nine are band 1; then per channel 12 values, 5 of band 2 and 7 of band 3
BAND = np.array([0] * 9 + [1 if (h - 9) % 12 < 5 else 2 for h in range(9, 45)])
# column of the PLY's f_rest property block (channel-major: f_rest[c * 15 + k - 1], k = 1..15) that lands in REST[h]
PLY_OF_REST = np.array([(h // 3) * 15 + h % 3 if h < 9 else ((h - 9) // 12) * 15 + (h - 9) % 12 + 3 for h in range(45)])


def quantise(aos):
    """(codes int8 (n, 45) in REST order, steps float32 (n, 3)) of 61-float records"""
    a = np.asarray(aos, np.float32)
    c = a[:, REST]
    codes = np.zeros(c.shape, np.int8)
    steps = np.zeros((c.shape[0], 3), np.float32)
    with np.errstate(all="ignore"):
        for b in range(3):
            cb = c[:, BAND == b]
            m = np.abs(cb).max(axis=1)
            assert m.dtype == np.float32
            live = m >= np.float32(2.0 ** -64)
            step = np.where(live, m / np.float32(127.0), np.float32(0.0)).astype(np.float32)
            q = cb / np.where(live, step, np.float32(1.0))[:, None]
            assert q.dtype == np.float32
            code = np.clip(np.rint(q), -127.0, 127.0)
            code = np.where(live[:, None] & np.isfinite(code), code, 0.0)
            codes[:, BAND == b] = code.astype(np.int8)
            steps[:, b] = step
    return codes, steps


def deq(aos):
    """the cloud SH_Q8 storage renders and downloads: f_rest = code * step, every other float unchanged"""
    out = np.array(aos, np.float32, copy=True)
    if out.shape[1] != 61:
        return out                                   # a degree-1 cloud is stored FP32
    codes, steps = quantise(out)
    with np.errstate(all="ignore"):
        out[:, REST] = codes.astype(np.float32) * steps[:, BAND]
    assert out.dtype == np.float32
    return out


def special_rest():
    """hand-made f_rest rows (k, 45) in REST order: every band of every row is one of the quantiser's edge cases"""
    f = np.float32

    def band_rows(nb):
        rows = []
        z = np.zeros(nb, np.float32)
        rows.append(z.copy())                                                    # all zeros: step 0
        r = z.copy(); r[nb // 2] = f(0.3); rows.append(r)                        # one non-zero value: code 127, the rest 0
        r = (np.linspace(-1.0, 0.5, nb)).astype(np.float32); rows.append(r)      # the maximum has a negative sign: code -127
        # exact ties c = (k + 0.5) * step, k even and odd, both signs: m = 127 makes step exactly 1
        r = z.copy(); r[:9] = [127.0, 2.5, 3.5, -2.5, -3.5, 0.5, -0.5, 125.5, 126.5]; rows.append(r)
        # ... and with step = 2^-10
        r = z.copy(); r[:9] = np.array([127.0, 2.5, 3.5, -2.5, -3.5, 0.5, -0.5, 125.5, 126.5], np.float32) * f(2.0 ** -10)
        rows.append(r)
        r = z.copy(); r[0] = f(0.25); r[1] = f(-0.0); r[2] = f(-1e-9); rows.append(r)     # -0.0 and a value far below step / 2
        r = z.copy(); r[1] = f(2.0 ** -65); r[2] = f(-2.0 ** -70); rows.append(r)        # maximum 2^-65: step 0
        r = z.copy(); r[1] = f(-2.0 ** -64); r[2] = f(2.0 ** -65); r[3] = f(2.0 ** -72); rows.append(r)     # maximum 2^-64: quantised
        r = (np.linspace(-0.7, 1.0, nb) * 1e30).astype(np.float32); rows.append(r)        # a band at 1e30
        r = z.copy(); r[0] = f(1e-38); r[1] = f(1e-40); r[2] = f(-3e-39); rows.append(r)  # subnormal values below a tiny maximum
        r = (np.linspace(-1.0, 1.0, nb) ** 3 * 0.15).astype(np.float32); rows.append(r)   # an ordinary band
        return rows

    per_band = [band_rows(int((BAND == b).sum())) for b in range(3)]
    k = len(per_band[0])
    out = np.zeros((k * 3, 45), np.float32)
    for shift in range(3):                       # every case in every band, next to two different neighbours
        for i in range(k):
            for b in range(3):
                out[shift * k + i, BAND == b] = per_band[b][(i + shift * b) % k]
    return out
