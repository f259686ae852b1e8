#!/usr/bin/env python3
"""Error of the quick-GELU of the FC1 epilogue (common.h quick_gelu / quick_gelu2xN, EPI_QGELU16) against float64 over [-12, 12].

The device form is x * rcp(1 + exp2(x * K)), K = fp32(-1.702 log2 e), every step rounded to fp32.  v_exp_f32 and v_rcp_f32 are good to 1 ulp,
not correctly rounded, so beside the correctly rounded emulation the script takes both results 1 ulp off, in each of the four sign
combinations, and reports the worst.  The bound to stay inside is the 1.7e-6 gelu_erf_fast documents (tools/gelu_fit.py).  CPU only."""
import numpy as np

K = np.float32(-1.702 * np.log2(np.e))
f32 = np.float32


def quick_gelu_f32(x, de=0, dr=0):
    """fp32 emulation; de / dr: ulps added to the exp2 / rcp results"""
    t = (x * K).astype(f32)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp2(t.astype(np.float64)).astype(f32)
    if de:
        e = np.nextafter(e, f32(np.inf) * de).astype(f32)
    d = (f32(1.0) + e).astype(f32)
    with np.errstate(divide="ignore"):
        r = (1.0 / d.astype(np.float64)).astype(f32)
    if dr:
        # 1 ulp of the EXACT result: 1 / d <= 1 for d >= 1 and its ulp is 2^-24 there, so a result 1 ulp off never exceeds 1.0
        # (nextafter(1.0, inf) would be 2 of those ulps away)
        r = np.minimum(np.nextafter(r, f32(np.inf) * dr), f32(1.0)).astype(f32)
    return (x * r).astype(f32)


def main():
    x = np.linspace(-12, 12, 4000001).astype(f32)
    x64 = x.astype(np.float64)
    exact = x64 / (1.0 + np.exp(-1.702 * x64))
    print(f"K = {K!r}")
    worst = 0.0
    for de, dr in ((0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        err = np.abs(quick_gelu_f32(x, de, dr).astype(np.float64) - exact)
        i = int(err.argmax())
        print(f"exp2 {de:+d} ulp, rcp {dr:+d} ulp: max |error| {err[i]:.3e} at x = {x[i]:.4f}")
        worst = max(worst, float(err[i]))
    # saturation: far outside the range the result is x or -0, never nan
    far = quick_gelu_f32(np.array([-1e4, -100.0, 100.0, 1e4], dtype=f32))
    print("far values", far)
    assert np.array_equal(far, np.array([-0.0, -0.0, 100.0, 1e4], dtype=f32)), far
    assert worst <= 1.7e-6, worst
    print(f"worst {worst:.3e} <= 1.7e-6 (gelu_erf_fast)")


if __name__ == "__main__":
    main()
