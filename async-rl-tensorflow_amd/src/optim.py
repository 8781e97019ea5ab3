"""RMSPropOptimizer with TF1 semantics (main.py:63-65 ``tf.train.RMSPropOptimizer(lr_op,
decay=0.99, momentum=0, epsilon=0.1)``): rms slot initialised to 1.0, momentum slot to 0,
ms += (g^2 - ms)(1 - decay); mom = mom*momentum + lr*g/sqrt(ms + epsilon); w -= mom, with the
per-tensor clip_by_norm of agent.py:316-319 fused in (a3c_clip_rmsprop_apply).  Works on a flat
fp32 parameter buffer + the tensor table of the C-ABI layout."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_handle


class RMSPropOptimizer(object):
  def __init__(self, learning_rate, decay=0.9, momentum=0.0, epsilon=1e-10, clip_norm=40.0):
    self.learning_rate = learning_rate      # float, or a callable returning the current lr (lr_op)
    self.decay, self.momentum, self.epsilon = float(decay), float(momentum), float(epsilon)
    self.clip_norm = float(clip_norm)
    self._slots = {}

  def slots(self, flat):
    key = flat.data_ptr()
    if key not in self._slots:
      self._slots[key] = (torch.ones_like(flat), torch.zeros_like(flat))
    return self._slots[key]

  def lr(self):
    return float(self.learning_rate() if callable(self.learning_rate) else self.learning_rate)

  def _ws(self, like):
    b = _lib.c_i64()
    check(lib().a3c_optim_workspace_bytes(int(like.numel()), ctypes.byref(b)), 'a3c_optim_workspace_bytes')
    return torch.empty(int(b.value), dtype=torch.uint8, device=like.device)

  def clip_only(self, flat_grads, offsets, sizes, sumsq=None):
    """Per-tensor clip_by_norm in place (each worker before the multi-GPU SUM all-reduce)."""
    check(lib().a3c_clip_grads(ptr(flat_grads), len(offsets), _lib.i64_array(offsets), _lib.i64_array(sizes),
                               self.clip_norm, ptr(sumsq), ptr(self._ws(flat_grads)), stream_handle()),
          'a3c_clip_grads')

  def apply_gradients(self, flat_params, flat_grads, offsets, sizes, lr=None, sumsq=None, clip=True):
    """clip (unless clip=False: already clipped per worker) + RMSProp apply."""
    ms, mom = self.slots(flat_params)
    ws = self._ws(flat_params)
    check(lib().a3c_clip_rmsprop_apply(ptr(flat_params), ptr(ms), ptr(mom), ptr(flat_grads), len(offsets),
                                       _lib.i64_array(offsets), _lib.i64_array(sizes),
                                       float(self.lr() if lr is None else lr), self.decay, self.momentum,
                                       self.epsilon, self.clip_norm if clip else 0.0, ptr(sumsq), ptr(ws), stream_handle()),
          'a3c_clip_rmsprop_apply')


def check_adam(beta1, beta2, epsilon):
  """Adam's constants as floats; ValueError where a3c_engine_set_optimizer would reject them."""
  beta1, beta2, epsilon = float(beta1), float(beta2), float(epsilon)
  if not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0):
    raise ValueError('adam_beta1 and adam_beta2 must lie in [0, 1): %r, %r' % (beta1, beta2))
  if not epsilon > 0.0:
    raise ValueError('adam_epsilon must be > 0: %r' % (epsilon,))
  return beta1, beta2, epsilon


def adam_alpha(lr, beta1_power, beta2_power):
  """TF1 ApplyAdam's step size: the fp32 lr times sqrt(1 - beta2^t) / (1 - beta1^t) in fp64, as fp32."""
  return float(np.float32(np.float64(np.float32(lr)) * np.sqrt(1.0 - np.float64(beta2_power))
                          / (1.0 - np.float64(beta1_power))))


class AdamOptimizer(RMSPropOptimizer):
  """tf.train.AdamOptimizer with TF1 ApplyAdam semantics behind RMSPropOptimizer's
  methods: m and v slots initialised to 0 and, per parameter buffer, the fp64 running products
  beta1^t, beta2^t.  Step t: alpha = lr * sqrt(1 - beta2^t) / (1 - beta1^t);
  m += (g - m)(1 - beta1); v += (g^2 - v)(1 - beta2); w -= m * alpha / (sqrt(v) + epsilon), with the
  per-tensor clip_by_norm fused in (a3c_clip_adam_apply).  ``slots`` returns (v, m): the places of
  RMSProp's (ms, mom), as in the engine."""

  def __init__(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8, clip_norm=40.0):
    self.learning_rate = learning_rate      # float, or a callable returning the current lr (lr_op)
    self.beta1, self.beta2, self.epsilon = check_adam(beta1, beta2, epsilon)
    self.clip_norm = float(clip_norm)
    self._slots = {}
    self._powers = {}

  def slots(self, flat):
    key = flat.data_ptr()
    if key not in self._slots:
      self._slots[key] = (torch.zeros_like(flat), torch.zeros_like(flat))
      self._powers[key] = [1.0, 1.0]
    return self._slots[key]

  def powers(self, flat):
    """[beta1^t, beta2^t] of the t steps applied to this buffer (the list itself: a checkpoint
    restores it in place)."""
    self.slots(flat)
    return self._powers[flat.data_ptr()]

  def apply_gradients(self, flat_params, flat_grads, offsets, sizes, lr=None, sumsq=None, clip=True):
    """clip (unless clip=False: already clipped per worker) + one Adam step."""
    v, m = self.slots(flat_params)
    pw = self.powers(flat_params)
    p1, p2 = pw[0] * self.beta1, pw[1] * self.beta2
    ws = self._ws(flat_params)
    check(lib().a3c_clip_adam_apply(ptr(flat_params), ptr(m), ptr(v), ptr(flat_grads), len(offsets),
                                    _lib.i64_array(offsets), _lib.i64_array(sizes),
                                    adam_alpha(self.lr() if lr is None else lr, p1, p2), self.beta1, self.beta2,
                                    self.epsilon, self.clip_norm if clip else 0.0, ptr(sumsq), ptr(ws), stream_handle()),
          'a3c_clip_adam_apply')
    pw[0], pw[1] = p1, p2
