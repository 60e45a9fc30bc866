"""Linear warm-up and polynomial decay of the learning rates.

The factor is a pure function of the optimizer step about to be taken: s = 1 is the first training step of the run and s counts
across epochs.  With W = --lr-num-warmup-steps, S0 = --lr-decay-start-step and N = --lr-num-decay-steps:

    s < W                       s / W
    else, N == 0 or s < S0      1
    else                        ((N - d) / N)^2,  d = min(s - S0, N - 1)

so behind the decay the factor stays at the last decay step's value, 1 / N^2.  One factor scales both --learning-rate and
--lr-embeds.  The flag names are the upstream DLRM's; the definition is this project's own.
"""
from __future__ import annotations

import ctypes as C

import numpy as np


class RateCell(C.c_float):
    """A rate argument that is patched per step instead of recorded by value: the engine hands one of these to `ops.*`, which
    passes it through to the library call where it would call float() on a number, so a recorded step keeps the OBJECT and a
    launch tape can tell a rate from any other float argument by identity.  It also stands in for a number where host code
    (a test double of `ops`) negates or multiplies the rate."""

    def __float__(self):
        return float(self.value)

    def __neg__(self):
        return -float(self.value)

    def __mul__(self, other):
        return float(self.value) * other

    __rmul__ = __mul__


def rate_arg(lr):
    """What `ops.*` hands the library for a rate: the cell itself, or the number as a float."""
    return lr if isinstance(lr, C.c_float) else float(lr)


def check(warmup_steps: int, decay_start_step: int, num_decay_steps: int) -> None:
    """What the schedule refuses, as one ValueError (the command line turns it into its ERROR: line)."""
    W, S0, N = int(warmup_steps), int(decay_start_step), int(num_decay_steps)
    for name, v in (("--lr-num-warmup-steps", W), ("--lr-decay-start-step", S0), ("--lr-num-decay-steps", N)):
        if v < 0:
            raise ValueError("%s=%d: not negative" % (name, v))
    if N > 0 and S0 < W:
        raise ValueError("--lr-decay-start-step=%d lies inside the warm-up (--lr-num-warmup-steps=%d): the warm-up has to end "
                         "before the decay starts" % (S0, W))


class LRSchedule:
    def __init__(self, warmup_steps: int = 0, decay_start_step: int = 0, num_decay_steps: int = 0):
        check(warmup_steps, decay_start_step, num_decay_steps)
        self.W, self.S0, self.N = int(warmup_steps), int(decay_start_step), int(num_decay_steps)

    @property
    def active(self) -> bool:
        return bool(self.W or self.S0 or self.N)

    def factor(self, s: int) -> float:
        """The factor of optimizer step s (1 = the run's first)."""
        s = int(s)
        if s < self.W:
            return s / self.W
        if self.N == 0 or s < self.S0:
            return 1.0
        d = min(s - self.S0, self.N - 1)
        return ((self.N - d) / self.N) ** 2

    def __repr__(self):
        return "LRSchedule(W=%d, S0=%d, N=%d)" % (self.W, self.S0, self.N)


def effective_rate(base: float, factor: float) -> np.float32:
    """The rate handed to the library: the ONE place that rounds base * factor to float32."""
    return np.float32(np.float64(base) * np.float64(factor))
