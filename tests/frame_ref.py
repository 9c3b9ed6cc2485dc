"""NumPy restatement of the frame recorder's definition (include/fibhip.h, fibhip_frames_*).  The device must equal it bit
for bit.  Every operation is a float32 operation rounded on its own, in the order the header states."""
import numpy as np

F32 = np.float32


def levels(min_v, max_v):
    """(lo, span) as a model's _frame_levels() rounds them: the subtraction in double, both rounded to float32"""
    return F32(min_v), F32(float(max_v) - float(min_v))


def out_shape(window, block):
    r0, r1, c0, c1 = window
    return (r1 - r0) // block[0], (c1 - c0) // block[1]


def cells(X, lo, span, weight=None):
    """y = (X - lo) / span, times the weight plane where one is given: [H, W] float32"""
    X = np.asarray(X, F32)
    with np.errstate(all='ignore'):
        y = (X - F32(lo)) / F32(span)
        if weight is not None:
            y = y * np.asarray(weight, F32)
    assert y.dtype == F32
    return y


def quantise(p):
    """U8: NaN -> 0, clamp to [0, 1], (unsigned char)(q * 255.0f + 0.5f), truncated"""
    p = np.asarray(p, F32)
    q = np.where(np.isnan(p), F32(0), p)
    q = np.minimum(np.maximum(q, F32(0)), F32(1))
    v = q * F32(255) + F32(0.5)
    assert v.dtype == F32
    return v.astype(np.uint8)


def frame(X, window=None, block=(1, 1), reduce='mean', lo=0.0, span=1.0, weight=None, fmt='float32'):
    """one frame of state array X ([H, W] float32): [oh, ow] float32 or uint8"""
    X = np.asarray(X, F32)
    H, W = X.shape
    r0, r1, c0, c1 = (0, H, 0, W) if window is None else window
    by, bx = block
    oh, ow = out_shape((r0, r1, c0, c1), block)
    assert oh >= 1 and ow >= 1
    y = cells(X, lo, span, weight)[r0:r0 + oh * by, c0:c0 + ow * bx]          # trailing cells are dropped
    blocks = y.reshape(oh, by, ow, bx)
    if reduce == 'point':
        pix = blocks[:, 0, :, 0].copy()
    else:
        with np.errstate(all='ignore'):
            total = None
            for dy in range(by):                                             # row sums, added top to bottom
                rs = blocks[:, dy, :, 0].copy()
                for dx in range(1, bx):                                      # each block row left to right
                    rs = rs + blocks[:, dy, :, dx]
                total = rs if total is None else total + rs
            pix = total / F32(by * bx)
    assert pix.dtype == F32 and pix.shape == (oh, ow)
    return quantise(pix) if fmt == 'uint8' else pix


def sample_ticks(every, first, ticks):
    """the tick numbers (counted from 1 at attach) a frame follows, among the first `ticks` ticks"""
    return list(range(first, ticks + 1, every))
