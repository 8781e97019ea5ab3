"""TF1 ApplyAdam as the engine applies it, restated in numpy.  Test infrastructure.

Per flat parameter vector: m = 0, v = 0 and two fp64 running products p1 = p2 = 1.  Once per applied step,
in fp64: p1 *= beta1; p2 *= beta2; alpha = (float)((double)lr * sqrt(1 - p2) / (1 - p1)), lr being the
float the schedule produces.  Per element, in fp32 with no contraction (numpy fuses nothing):

    omb1 = 1.0f - (float)beta1;  omb2 = 1.0f - (float)beta2
    m = m + (g - m) * omb1
    v = v + (g*g - v) * omb2
    w = w - (m * alpha) / (sqrtf(v) + (float)eps)

g is the per-tensor-clipped gradient.  eps sits outside the square root and is not scaled by the bias
correction: that is TF's placement (torch.optim.Adam divides by sqrt(v / (1 - p2)) + eps).

dtype=np.float64 evaluates the same expressions with every cast to float a cast to double (the comparison
with torch.optim.Adam in fp64)."""
import numpy as np

BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def alpha(lr, p1, p2, dtype=np.float32):
    """The step size of the step whose products (already advanced) are p1, p2."""
    return dtype(np.float64(dtype(lr)) * np.sqrt(np.float64(1.0) - np.float64(p2)) / (np.float64(1.0) - np.float64(p1)))


class Adam:
    """One optimizer over named (or one anonymous) parameter arrays sharing the two products."""

    def __init__(self, beta1=BETA1, beta2=BETA2, eps=EPS, dtype=np.float32):
        self.beta1, self.beta2, self.eps, self.dtype = float(beta1), float(beta2), float(eps), dtype
        self.p1 = self.p2 = 1.0                  # python floats: fp64
        self.m, self.v = {}, {}

    def advance(self):
        """The products of the next step; returns them (p1, p2)."""
        self.p1 *= self.beta1
        self.p2 *= self.beta2
        return self.p1, self.p2

    def update(self, key, w, g, a):
        """One element-wise step of array w (in place) with gradient g and step size a (this step's alpha)."""
        t = self.dtype
        g = np.asarray(g, t)
        if key not in self.m:
            self.m[key], self.v[key] = np.zeros(w.shape, t), np.zeros(w.shape, t)
        m, v = self.m[key], self.v[key]
        omb1, omb2 = t(1.0) - t(self.beta1), t(1.0) - t(self.beta2)
        m[...] = m + (g - m) * omb1
        v[...] = v + (g * g - v) * omb2
        w[...] = w - (m * t(a)) / (np.sqrt(v) + t(self.eps))

    def step(self, params, grads, lr):
        """One applied step of every array of the dict params (or of one array) with the float lr; returns alpha."""
        p1, p2 = self.advance()
        a = alpha(lr, p1, p2, self.dtype)
        if isinstance(params, dict):
            for k in params:
                self.update(k, params[k], grads[k], a)
        else:
            self.update(None, params, grads, a)
        return a

    def sequence(self, params, grads_seq, lr):
        """The partitioned PS: every gradient of grads_seq is a step of its own, in order, with one lr."""
        return [self.step(params, g, lr) for g in grads_seq]
