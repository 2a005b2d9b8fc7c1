"""NumPy restatement of the arithmetic of csrc/pwc_optim.hip (include/pwc_hip.h, pwc_optim_adam_update), operation by operation.

dtype = np.float32 is what the kernel computes, bit for bit; dtype = np.float64 is the same sequence in double, the form that is
compared with torch.optim.Adam / AdamW.  The clip coefficient is an INPUT (the norm is a separate pass with its own check), and the
step record {step, beta1^step, beta2^step} is carried as the running products the finish pass keeps, in double for either dtype.
"""
import math

import numpy as np


def clip_coef(total_norm, max_norm):
    """min(1, max_norm / (total_norm + 1e-6)) in float32, as pwc_optim_finish and torch's clip_grad_norm_ form it."""
    c = np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6))
    return np.float32(1.0) if c > np.float32(1.0) else c


class AdamOracle:
    def __init__(self, params, dtype=np.float32):
        self.dtype = np.dtype(dtype).type
        self.p = [np.array(p, dtype=dtype).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.step_count, self.b1_pow, self.b2_pow = 0, 1.0, 1.0

    def step(self, grads, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, coef=1.0, grad_scale=None,
             found_inf=False):
        """One step on the tensors whose gradient is not None.  coef: the clip coefficient; grad_scale: GradScaler's scale (the
        gradients are multiplied by fl(1 / scale)); found_inf: the step is skipped and the record does not advance."""
        if found_inf:
            return
        T = self.dtype
        b1, b2 = betas
        self.step_count += 1
        self.b1_pow *= b1                                        # Python floats: double
        self.b2_pow *= b2
        step_size = T(lr / (1.0 - self.b1_pow))                  # formed in double, rounded once
        bc2_sqrt = T(math.sqrt(1.0 - self.b2_pow))
        omb1, b2t, omb2, epst, wd, decay = T(1.0 - b1), T(b2), T(1.0 - b2), T(eps), T(weight_decay), T(1.0 - lr * weight_decay)
        inv_scale = T(1.0) if grad_scale is None else T(1.0) / T(grad_scale)
        coef = T(coef)
        for i, g in enumerate(grads):
            if g is None:
                continue
            p, m, v = self.p[i], self.m[i], self.v[i]
            g = np.asarray(g, dtype=T)
            g = g * inv_scale * coef
            if weight_decay != 0.0:
                if decoupled:
                    p = p * decay
                else:
                    g = g + wd * p
            m = m + omb1 * (g - m)
            v = v * b2t + omb2 * (g * g)
            p = p + (-step_size) * (m / (np.sqrt(v) / bc2_sqrt + epst))
            assert p.dtype == T and m.dtype == T and v.dtype == T
            self.p[i], self.m[i], self.v[i] = p, m, v
