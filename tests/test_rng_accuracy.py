"""CPU: the fp32 Box-Muller of the RNG contract (box_muller_f32 in pc-gym_amd/csrc/pcg_kernels.hpp, its C twin in
oracle/pcg_oracle.c) against a Box-Muller in np.longdouble.

The two statements are compared with EACH OTHER bit for bit (test_gpu_actor_rollout.test_noise_is_the_oracle_twin_bitwise,
tests/test_gpu_closed_loop_sharding.py for every closed-loop kernel family); a wrong coefficient of the hand-written ln / sin /
cos polynomials would be wrong on both sides.  Here the twin (orc_box_muller_f32_n: the static function on n word pairs) is held
against

    u0 = (((w0 >> 9) << 1) | 1) 2^-24,  u1 = (w1 >> 8) 2^-24          (exact)
    r = sqrt(-2 ln u0),  z0 = r cos(2 pi u1),  z1 = r sin(2 pi u1)     (np.longdouble)

on: every one of the 2^23 u0 values at the angle word 0x12345600; every 16th of the 2^24 angle values at w0 = 0 (the smallest
u0, the largest r) and at w0 = 0xFFFFFFFF (u0 next to 1, r ~ 3e-4); the words around m = sqrt(1/2), where the ln switches
its exponent, against every 256th angle; the quarter-turn seams of the angle (0xFFFFFF00 takes the n = 4 wrap) against every
128th u0; and 2^21 pairs from Philox4x32-10 under the engine's own keys (global env indices from 2^33 + 5, purpose 0x400).

Bar: |z - z_ref| <= 6 x 2^-24 x max(r, 2^-12) for both components -- the budget of the stated operation sequence: about 1.6
units from rounding a pi (a up to pi/4 times the float32 pi, then the error of a enters r sin / r cos with weight r), about 1
from r (ln and sqrt), about 0.4 from the truncated cosine series at pi/4, 0.5 from the final product.  The search that came
with the bar (2e8 random pairs, eleven edge words against every angle, every u0 at ten angles) found 3.41 units at worst, at
w0 = dfd77add, w1 = b6f022ab.  The floor 2^-12 covers r -> 0, where the absolute error of the series remains.  A sine
coefficient wrong in its fourth digit (8.33e-3 for 1/120) gives 18 units at w0 = 0.

Moments of the 2^21 random pairs, five-sigma bars of the standard normal itself: |mean| <= 5 / sqrt(n),
|var - 1| <= 5 sqrt(2 / n), |corr(z0, z1)| <= 5 / sqrt(n).

The device needs no test of its own for this: pcg_policy_noise == orc_rng_normal is asserted bitwise on the GPU, and
tests/test_gpu_closed_loop_sharding.py extends that to every closed-loop family.  Not reachable on the device: the edge words
(u0 = 2^-24 through the frexp builtins, the n = 4 wrap of the angle) cannot be forced through Philox.

Worst figures this test sees (it prints every sample's): 3.41 units = 2.04e-7 of r at that pair, which is part of the sample;
3.23 units = 1.93e-7 of r on the rest, at w0 = e13b6f82, w1 = 045a4989 (a Philox pair).
"""
import ctypes as C

import numpy as np

LD = np.longdouble
UNIT = 2.0 ** -24
BAR = 6.0
R_FLOOR = 2.0 ** -12
G = (1 << 33) + 5
M32 = np.uint64(0xFFFFFFFF)


def twin(w0, w1):
    """(z0, z1) float32 of the oracle's box_muller_f32 on the word pairs"""
    from oracle import oracle as O

    f = O.lib().orc_box_muller_f32_n
    f.restype = None
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    w0, w1 = np.ascontiguousarray(w0, dtype=np.uint32), np.ascontiguousarray(w1, dtype=np.uint32)
    assert w0.shape == w1.shape and w0.ndim == 1
    z0, z1 = np.empty(w0.size, dtype=np.float32), np.empty(w0.size, dtype=np.float32)
    f(w0.ctypes.data, w1.ctypes.data, w0.size, z0.ctypes.data, z1.ctypes.data)
    return z0, z1


def reference(w0, w1):
    """(r, z0, z1) in np.longdouble from the uniforms as the header states them"""
    u0 = (((w0.astype(np.uint32) >> np.uint32(9)) << np.uint32(1)) | np.uint32(1)).astype(LD) * LD(UNIT)
    u1 = (w1.astype(np.uint32) >> np.uint32(8)).astype(LD) * LD(UNIT)
    r = np.sqrt(LD(-2) * np.log(u0))
    ang = (LD(8) * np.arctan(LD(1))) * u1
    return r, r * np.cos(ang), r * np.sin(ang)


def philox_numpy(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Random123) on uint64 arrays holding 32-bit words"""
    c0, c1, c2, c3 = (np.asarray(v, dtype=np.uint64) & M32 for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def random_pairs(n_blocks, seed=0x1234567, purpose=0x400):
    """2 n_blocks word pairs the way rng_normal2 takes them from the blocks of global envs G, G + 1, ... at t = 0"""
    env = np.uint64(G) + np.arange(n_blocks, dtype=np.uint64)
    o = philox_numpy(env & M32, env >> np.uint64(32), 0, purpose, seed & 0xFFFFFFFF, seed >> 32)
    return np.concatenate([o[0], o[2]]).astype(np.uint32), np.concatenate([o[1], o[3]]).astype(np.uint32)


_WORST = {"units": 0.0}


def check(name, w0, w1):
    w0, w1 = (np.ascontiguousarray(np.broadcast_to(np.asarray(w, dtype=np.uint32), np.broadcast(w0, w1).shape)).ravel() for w in (w0, w1))
    z0, z1 = twin(w0, w1)
    r, r0, r1 = reference(w0, w1)
    scale = LD(UNIT) * np.maximum(r, LD(R_FLOOR))
    e0, e1 = (np.abs(z0.astype(LD) - r0) / scale).astype(np.float64), (np.abs(z1.astype(LD) - r1) / scale).astype(np.float64)
    err = np.maximum(e0, e1)
    assert np.isfinite(err).all(), name
    i = int(np.argmax(err))
    rel = float(err[i]) * UNIT * float(max(r[i], R_FLOOR)) / float(r[i])
    print(f"box_muller_f32 vs long double, {name}: {w0.size} pairs, worst {err[i]:.3f} units of 2^-24 max(r, 2^-12) = {rel:.3e} of r "
          f"(r = {float(r[i]):.4g}) at w0 = {int(w0[i]):08x}, w1 = {int(w1[i]):08x}")
    if err[i] > _WORST["units"]:
        _WORST.update(units=float(err[i]), rel=rel, w0=int(w0[i]), w1=int(w1[i]))
    assert err[i] <= BAR, f"{name}: {err[i]:.3f} units at w0 = {int(w0[i]):08x}, w1 = {int(w1[i]):08x} (bar {BAR:g})"
    return z0, z1


def test_numpy_philox_is_the_oracles():
    from oracle import oracle as O

    for ctr, key in (((0, 0, 0, 0), (0, 0)), ((5, 2, 7, 0x400), (0x1234567, 0)), ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF)),
                     ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))):
        got = [int(v[0]) for v in philox_numpy(*[np.array([c]) for c in ctr], *key)]
        assert got == O.philox(ctr, key), (ctr, key)
    # Random123's known-answer vectors
    assert [int(v[0]) for v in philox_numpy(*[np.array([0])] * 4, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_box_muller_f32_against_long_double():
    """the whole sample of the module docstring, one bar"""
    ANGLES16 = (np.arange(1 << 20, dtype=np.uint32) << np.uint32(12))     # every 16th of the 2^24 angle values
    ANGLES256 = (np.arange(1 << 16, dtype=np.uint32) << np.uint32(16))
    U0_ALL = (np.arange(1 << 23, dtype=np.uint32) << np.uint32(9))
    U0_128 = (np.arange(1 << 16, dtype=np.uint32) << np.uint32(16))
    SQRT_HALF = np.array([0xB504F300, 0xB504F400, 0x5A827900, 0x5A827A00], dtype=np.uint32)
    SEAMS = np.array([0, 0x20000000, 0x3FFFFF00, 0x40000000, 0x60000000, 0xDFFFFF00, 0xE0000000, 0xFFFFFF00], dtype=np.uint32)
    check("every u0 at the angle word 12345600", U0_ALL, np.uint32(0x12345600))
    z0, _ = check("w0 = 0 (u0 = 2^-24), every 16th angle", np.uint32(0), ANGLES16)
    assert float(np.max(np.abs(z0))) > 5.76, "u0 = 2^-24 gives r = sqrt(48 ln 2) = 5.768"
    z0, z1 = check("w0 = ffffffff (u0 = 1 - 2^-24), every 16th angle", np.uint32(0xFFFFFFFF), ANGLES16)
    assert 3.4e-4 < float(np.max(np.hypot(z0, z1))) < 3.5e-4
    check("the words around m = sqrt(1/2), every 256th angle", SQRT_HALF[:, None], ANGLES256[None, :])
    check("the words around m = sqrt(1/2) on the seams", SQRT_HALF[:, None], SEAMS[None, :])
    z0, z1 = check("the quarter-turn seams, every 128th u0", U0_128[None, :], SEAMS[:, None])
    # the seams are where a component vanishes: 0, 1/8, 1/4 - ulp, 1/4, 3/8, 7/8 - ulp, 7/8, 1 - ulp of a turn
    n = U0_128.size
    assert np.all(z1[:n] == 0) and np.all(z0[:n] > 0), "angle 0: z1 = 0, z0 = r"
    assert np.all(z0[3 * n:4 * n] == 0) and np.all(z1[3 * n:4 * n] > 0), "a quarter turn: z0 = 0, z1 = r"
    assert np.all(z0[7 * n:] > 0) and np.all(z1[7 * n:] < 0) and np.all(np.abs(z1[7 * n:]) < 1e-5), "one 2^-24 turn below a full turn (n = 4)"
    check("the worst pair of the 2e8-pair search", np.array([0xDFD77ADD], dtype=np.uint32), np.array([0xB6F022AB], dtype=np.uint32))
    w0, w1 = random_pairs(1 << 20)
    z0, z1 = check("2^21 Philox pairs", w0, w1)
    print(f"box_muller_f32 vs long double: worst of all samples {_WORST['units']:.2f} units of 2^-24 max(r, 2^-12) = {_WORST['rel']:.2e} of r "
          f"at w0 = {_WORST['w0']:08x}, w1 = {_WORST['w1']:08x} (bar {BAR:g} units)")

    # ---- moments of the random sample: five-sigma bars of the standard normal ----
    n = z0.size
    assert n == 1 << 21
    z0, z1 = z0.astype(np.float64), z1.astype(np.float64)
    for name, z in (("z0", z0), ("z1", z1)):
        mean, var = float(np.mean(z)), float(np.var(z))
        print(f"{name}: mean {mean:+.3e} (bar {5 / np.sqrt(n):.3e}), var - 1 {var - 1:+.3e} (bar {5 * np.sqrt(2 / n):.3e})")
        assert abs(mean) <= 5 / np.sqrt(n), (name, mean)
        assert abs(var - 1) <= 5 * np.sqrt(2 / n), (name, var)
    corr = float(np.corrcoef(z0, z1)[0, 1])
    print(f"corr(z0, z1) {corr:+.3e} (bar {5 / np.sqrt(n):.3e})")
    assert abs(corr) <= 5 / np.sqrt(n), corr
