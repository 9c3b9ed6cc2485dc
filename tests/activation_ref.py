"""NumPy restatement of the activation recorder (include/fibhip.h fibhip_observe_*, csrc/record_kernels.inc observe_kernel):
feed it the watched array after every tick and it keeps the same five maps, bit for bit."""
import numpy as np


class ActivationRef:
    def __init__(self, v0, up, down, dt, steps_per_tick):
        self.vp = np.array(v0, np.float32)
        self.up, self.down = np.float32(up), np.float32(down)
        self.dt, self.spt = float(dt), int(steps_per_tick)
        self.tick = np.float32(self.dt * self.spt)
        shape = self.vp.shape
        self.first_up = np.full(shape, np.nan, np.float32)
        self.last_up = np.full(shape, np.nan, np.float32)
        self.prev_up = np.full(shape, np.nan, np.float32)
        self.apd = np.full(shape, np.nan, np.float32)
        self.count = np.zeros(shape, np.int32)
        self.k = 0

    def step(self, vc):
        """observed tick k: `vc` is the watched array after it"""
        vc = np.array(vc, np.float32)
        vp, up, down, tick = self.vp, self.up, self.down, self.tick
        t0 = np.float32(float(self.k) * self.dt * self.spt)         # (float)((double)k * dt * steps_per_tick)
        with np.errstate(all='ignore'):
            rise = (vp < up) & (vc >= up)
            fall = (vp >= down) & (vc < down) & (self.count > 0)
            t_up = t0 + ((up - vp) / (vc - vp)) * tick
            t_down = t0 + ((vp - down) / (vp - vc)) * tick
            self.apd[fall] = t_down[fall] - self.last_up[fall]
        self.prev_up[rise] = self.last_up[rise]
        self.last_up[rise] = t_up[rise]
        first = rise & (self.count == 0)
        self.first_up[first] = t_up[first]
        self.count[rise] += 1
        self.vp = vc
        self.k += 1

    def maps(self):
        return {'first_up': self.first_up.copy(), 'last_up': self.last_up.copy(), 'prev_up': self.prev_up.copy(),
                'apd': self.apd.copy(), 'count': self.count.copy()}


def bit_equal(a, b):
    """same shape and the same bits everywhere (NaN positions included)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int32), b.view(np.int32))
