"""Child process of test_gpu_ops.test_conv3x3_without_halo_kernel (not collected by pytest).

CNNITMO_HALO is read once per process, so the implicit-GEMM fallback of the 3x3 conv
(igemm_fwd_kernel, igemm_fwd2_kernel: conv_route() in conv_dispatch.hip) needs a process of its own.
With CNNITMO_HALO=0 this runs the existing checks, imported and not copied, at their own bounds:

  * test_gpu_ops.conv3x3_case (test_conv3x3_fwd_dgrad_wgrad's body) on kernel_cases.CONV3X3_HALO0;
  * test_gpu_ops.affine_epilogue_case (test_conv_affine_inference_epilogue's body) on AFFINE_HALO0;
  * test_gpu_exact.conv3x3_exact and affine_exact (the bit-for-bit cases on integer operands,
    tests/exact_cases.py) on the same two lists, both regimes;
  * test_gpu_model.test_unet_train_step_parity, both dtypes.

Every 3x3 conv launch goes through ops.call: its kernel name is asked first and must start with
"igemm_"; the entry points only the halo kernel implements must not be launched at all.  The
first failure ends the process (an exception: exit status 1).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HALO_ONLY = ("cnnitmo_conv3x3_fwd_pool", "cnnitmo_conv3x3_fwd_head", "cnnitmo_conv3x3_fwd_cat",
             "cnnitmo_conv3x3_dgrad_bn", "cnnitmo_conv3x3_dgrad_bn_pooled")


def main():
    assert os.environ.get("CNNITMO_HALO") == "0", "run with CNNITMO_HALO=0"
    t0 = time.time()
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from cnn_itmo_amd import _lib as L
    from cnn_itmo_amd import ops
    from tests import kernel_cases as KC
    from tests import exact_cases as E
    from tests import test_gpu_exact as X
    from tests import test_gpu_model as M
    from tests import test_gpu_ops as T

    seen = {}
    real = ops.call

    def call(name, *a):
        nm = None
        if name == "cnnitmo_conv3x3_fwd":
            dt, n, h, w, cin, cout = a[0], a[4], a[5], a[6], a[7], a[10]
            nm = L.query("cnnitmo_conv3x3_kernel_name", dt, n, h, w, cin, cout, 0).decode()
        elif name == "cnnitmo_conv3x3_dgrad":
            dt, n, h, w, cout, cin = a[0], a[2], a[3], a[4], a[5], a[7]
            nm = L.query("cnnitmo_conv3x3_kernel_name", dt, n, h, w, cin, cout, 1).decode()
        assert name not in HALO_ONLY, f"{name} launched with the halo kernel switched off"
        if nm is not None:
            assert nm.startswith("igemm_"), f"{name} {a[:11]}: {nm}"
            seen[nm] = seen.get(nm, 0) + 1
        return real(name, *a)

    ops.call = call
    for (cin, cout, h, w), names in KC.CONV3X3_HALO0.items():
        for dt in ("f32", "bf16"):
            assert all(nm.startswith("igemm_") for nm in names[dt][:2]), names[dt]
            T.conv3x3_case(dt, cin, cout, h, w, names[dt])
            print(f"conv3x3 {cin}->{cout} {h}x{w} {dt}: fwd {names[dt][0]}, dgrad {names[dt][1]}, "
                  f"wgrad {names[dt][2]}: ok", flush=True)
    for (dt, h, w, cin, cout), name in KC.AFFINE_HALO0.items():
        T.affine_epilogue_case(dt, h, w, cin, cout, name)
        print(f"affine epilogue {cin}->{cout} {h}x{w} {dt}: {name}: ok", flush=True)
    for regime in E.REGIMES:
        for (cin, cout, h, w), names in KC.CONV3X3_HALO0.items():
            for dt in ("f32", "bf16"):
                X.conv3x3_exact(dt, cin, cout, h, w, regime, names[dt])
                print(f"exact {regime} conv3x3 {cin}->{cout} {h}x{w} {dt}: fwd {names[dt][0]}, dgrad {names[dt][1]}: "
                      "every bit", flush=True)
        for (dt, h, w, cin, cout), name in KC.AFFINE_HALO0.items():
            X.affine_exact(dt, h, w, cin, cout, regime, name)
            print(f"exact {regime} affine epilogue {cin}->{cout} {h}x{w} {dt}: {name}: every bit", flush=True)
    cases = dict(seen)
    for dtype in ("float32", "bfloat16"):
        M.test_unet_train_step_parity(dtype)
        print(f"unet train step parity {dtype}: ok", flush=True)
    step = {k: v - cases.get(k, 0) for k, v in seen.items() if v > cases.get(k, 0)}
    print("conv launches of the two training steps:", step)
    print("conv launches by kernel:", seen)
    assert len(step) >= 4, step
    print(f"halo0 child ok in {time.time() - t0:.1f} s", flush=True)


if __name__ == "__main__":
    main()
