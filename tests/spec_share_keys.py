"""The spectral key of an event (csrc/gen_share.h, specshare), restated for the tests.

Two float32-chain events get the same grain from the spectral kernels when they read
the same micro grain (equal generator keys), every EventRt field the chain reads is
equal as bits, and each alone would run the same kernel.  The first event in list
order with a key is its owner; an event that writes micro_last (the last event of a
tilt-mode preset) always runs, and owns its key only when it is the first.
"""
import math
import struct

from msgpu import _lib as L

SPEC_TILT_NOISE, SPEC_TILT_SKEW, SPEC_LOWPASS, SPEC_STRETCH, SPEC_WARP = 1, 2, 4, 8, 16
TILT = SPEC_TILT_NOISE | SPEC_TILT_SKEW


def _bits(x):
    return struct.pack("<d", float(x))


def spec_ops(s, e):
    """EventRt::ops of event e of the packed preset s."""
    ops = 0
    if s.gen_mode in (L.GEN_MODE["Noise burst"], L.GEN_FALLBACK):
        ops |= SPEC_TILT_NOISE
    if s.gen_mode == L.GEN_MODE["Skewed transient"]:
        ops |= SPEC_TILT_SKEW
    if (s.flags & L.F_BANDLIMIT) and e.n >= 8:
        ops |= SPEC_LOWPASS
    if (s.flags & L.F_NL_WARP) and e.n >= 16:
        ops |= SPEC_WARP
    if not (s.flags & L.F_PARTIAL_LOCK) and e.n >= 16 and abs(e.stretch - 1.0) >= 1e-9:
        ops |= SPEC_STRETCH
    return ops


def generator_key(s, e):
    mode = 2 if s.gen_mode == L.GEN_FALLBACK else s.gen_mode       # Noise burst, MS:686
    return ((s.seed + e.index) & (2 ** 64 - 1), e.n, e.gen_sr, mode, _bits(s.ring_hz), _bits(s.ring_decay_ms),
            _bits(s.micro_ms))


def spectral_key(s, e):
    """Generator key + the chain's parameters + the kernel class.  tilt_alpha and env_tau are
    functions of the preset's tilt and (micro_ms, mode), computed as the library does.  The
    kernel an event runs is a function of these fields alone for the lengths the tests use
    (even n: every grain offset is even), except that ops == 0 is the copy."""
    ops = spec_ops(s, e)
    tilt = -3.0 if s.gen_mode == L.GEN_FALLBACK else s.noise_tilt
    tilt_alpha = math.log(math.pow(10.0, tilt / 20.0)) / math.log(2.0)
    env_tau = max(1e-6, (s.micro_ms / 1000.0) * (0.2 if s.gen_mode == L.GEN_MODE["Skewed transient"] else 0.25))
    return generator_key(s, e) + (ops, _bits(e.cutoff_out * e.ufac), _bits(s.bandlimit_roll_hz), _bits(e.stretch),
                                  _bits(tilt_alpha), _bits(env_tau), _bits(s.nl_warp_power), ops == 0)


def expected(presets, events, base, count):
    """Per slot its spectral owner, the events that run, the distinct keys and the distinct
    generator keys, by dictionaries over the full keys."""
    first, own, gen = {}, {}, set()
    for p, s in enumerate(presets):
        for k in range(count[p]):
            slot = base[p] + k
            e = events[slot]
            key = spectral_key(s, e)
            gen.add(generator_key(s, e))
            o = first.setdefault(key, slot)
            must_run = k == count[p] - 1 and (spec_ops(s, e) & TILT)
            own[slot] = slot if must_run else o
    runs = sum(1 for slot, o in own.items() if o == slot)
    return own, runs, len(first), len(gen)
