"""Child processes of test_abi_and_host.py's host-query tests (not collected by pytest).

    python tests/host_query_child.py sweep     every host-only query over the argument grid
    python tests/host_query_child.py values    the sweep's calls as "name(args) -> value" lines, with
                                               n = 32 at the U-Net frame sizes and channel
                                               counts up to 512 added: diff two libraries' output
    python tests/host_query_child.py launch    wgrad launches with channel counts below 32
    python tests/host_query_child.py names     kernel names as JSON (tests/kernel_cases.py),
                                               under whatever CNNITMO_HALO the parent set
    python tests/host_query_child.py exact_names   the same for the bit-exact cases
                                               (tests/exact_cases.py: launched)

Each call is printed before it is made (unbuffered), so that after a signal the parent can
report the last line as the call that killed the process.  The library is loaded through
ctypes alone: no torch, no device tensor.
"""
import ctypes
import importlib.util
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cnn_itmo.h")
QUERY = re.compile(r"cnnitmo_\w*(_rows|_workspace_bytes|_supported|_kernel_name)$")

CH = (0, 1, 3, 8, 16, 24, 32, 40, 48, 64, 96, 128)
HW = ((1, 1), (6, 10), (16, 64))
M = (0, 1, 255, 1000)
# added in the values mode: the bench's layers (n = 32 at each U-Net level) and wide layers
UNET_HW = ((1088, 1920), (544, 960), (272, 480), (136, 240), (68, 120))
CH_WIDE = CH + (160, 192, 256, 384, 512)
# values of the parameters that are not part of a joint grid below, by their name in the header
SINGLE = {"dtype": (0, 1), "n": (2,), "ntaps": (1, 4, 9), "dgrad": (0, 1), "with_grad": (0, 1), "scales": (1, 5),
          "m": M, "p": M, "rows": M, "ncols": CH, "c": CH, "cols": CH}


def load_lib():
    """cnn_itmo_amd/_lib.py by path: the package itself would import torch."""
    spec = importlib.util.spec_from_file_location("_cnnitmo_lib", os.path.join(ROOT, "cnn_itmo_amd", "_lib.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod, mod.load()


def header_params():
    """{entry point: [parameter names]} from include/cnn_itmo.h."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", "", txt)
    out = {}
    for m in re.finditer(r"\b(cnnitmo_\w+)\s*\(([^)]*)\)\s*;", txt):
        args = [a.strip() for a in m.group(2).split(",")]
        out[m.group(1)] = [] if args in ([""], ["void"]) else [re.findall(r"\w+", a)[-1] for a in args]
    return out


def grid(params, ch=CH, hw=HW, n=None):
    """Argument tuples of one query: the product of its parameters' values.  Channel counts
    go through the whole ch x ch grid; c1 (the first concat member) and the fused column range
    (c0, c1) take a few values of their own.  n: the batch sizes (default: SINGLE's)."""
    axes = []
    names = list(params)
    fused = "c0" in names
    for p in names:
        if p in ("h", "w"):
            continue
        if p in ("cin", "cout"):
            axes.append(ch)
        elif p == "n" and n is not None:
            axes.append(n)
        elif p == "c0":
            axes.append((0, 32))
        elif p == "c1":
            axes.append((-1, 0, 32) if fused else (0, 32, 64))  # -1: cin (every column above c0)
        else:
            axes.append(SINGLE[p])  # KeyError: a new query parameter needs its values here
    shapes = hw if "h" in names else ((None, None),)

    def rec(i, acc):
        if i == len(axes):
            yield tuple(acc)
            return
        for v in axes[i]:
            yield from rec(i + 1, acc + [v])

    rest = [p for p in names if p not in ("h", "w")]
    for h, w in shapes:
        for vals in rec(0, []):
            d = dict(zip(rest, vals))
            if fused and d["c1"] == -1:
                d["c1"] = d["cin"]
            d["h"], d["w"] = h, w
            yield tuple(d[p] for p in names)


def say(line):
    os.write(1, (line + "\n").encode())


def sweep():
    L, lib = load_lib()
    params = header_params()
    calls = 0
    for name in sorted(L.SIGNATURES):
        if not QUERY.search(name):
            continue
        res, argt = L.SIGNATURES[name]
        assert all(t in (L.i32, L.i64) for t in argt), f"{name}: a host-only query takes integers only"
        assert len(params[name]) == len(argt), name
        fn = getattr(lib, name)
        for args in grid(params[name]):
            say(f"{name}{args}")
            v = fn(*args)
            calls += 1
            if res is ctypes.c_char_p:
                assert v is not None, (params[name], args)
            if unsupported(name, dict(zip(params[name], args))):
                assert not v, f"{name}{args} -> {v!r} for channel counts that no launch takes"
    say(f"done {calls}")


def values():
    L, lib = load_lib()
    params = header_params()
    for name in sorted(L.SIGNATURES):
        if not QUERY.search(name):
            continue
        fn = getattr(lib, name)
        calls = list(grid(params[name], CH_WIDE))
        if "h" in params[name] and "n" in params[name]:
            calls += grid(params[name], CH_WIDE, UNET_HW, (32,))
        say("\n".join(f"{name}{args} -> {fn(*args)!r}" for args in calls))


def unsupported(name, d):
    """Channel counts every launch behind this query refuses with CNNITMO_EINVAL: the query gives
    0 bytes, 0 rows, "" or 0 (not supported).  A zero count launches nothing anywhere; the weight
    gradients (run_wgrad) need multiples of 32 on both sides, the 3x3 conv (launch_fwd,
    launch_fwd2, halo_plan) a multiple of 32 output columns (cout forward, cin for the dgrad)."""
    ci, co = d.get("cin"), d.get("cout")
    if ci is None or co is None:
        return False
    if ci <= 0 or co <= 0:
        return True
    if name in ("cnnitmo_wgrad_workspace_bytes", "cnnitmo_tconv2x2_wgrad_workspace_bytes", "cnnitmo_wgrad_kernel_name"):
        return ci % 32 != 0 or co % 32 != 0
    if name in ("cnnitmo_conv3x3_kernel_name", "cnnitmo_conv3x3_stat_rows"):
        return (ci if d.get("dgrad") else co) % 32 != 0
    return False


def launch():
    """cnnitmo_conv_wgrad / cnnitmo_tconv2x2_wgrad with channel counts below 32: run_wgrad's
    CNN_REQUIRE on the channel counts comes before any workspace use or launch, and the halo /
    row-streaming launchers before it refuse such sizes on the host, so the dummy pointers are
    never dereferenced and nothing is launched."""
    L, lib = load_lib()
    dummy = (ctypes.c_char * 4096)()
    p = ctypes.cast(dummy, ctypes.c_void_p)
    calls = 0
    for dt in (0, 1):
        for cin, cout in ((3, 32), (32, 8), (16, 16), (24, 64), (64, 24), (0, 32), (32, 0)):
            for ntaps in (1, 9):
                say(f"cnnitmo_conv_wgrad(dtype={dt}, ntaps={ntaps}, cin={cin}, cout={cout})")
                rc = lib.cnnitmo_conv_wgrad(dt, ntaps, p, max(cin, 8), 0, p, 2, 6, 10, cin, cout, p, 0, None, None, None,
                                            None, None, p, 4096, None)
                msg = lib.cnnitmo_last_error()
                assert rc < 0 and msg, (rc, msg)
                calls += 1
            say(f"cnnitmo_tconv2x2_wgrad(dtype={dt}, cin={cin}, cout={cout})")
            rc = lib.cnnitmo_tconv2x2_wgrad(dt, p, p, 2, 6, 10, cin, cout, p, None, None, None, None, p, 4096, None)
            msg = lib.cnnitmo_last_error()
            assert rc < 0 and msg, (rc, msg)
            calls += 1
    say(f"done {calls}")


def names():
    sys.path.insert(0, ROOT)
    from tests import kernel_cases as KC
    _, lib = load_lib()
    q = lambda name, *a: getattr(lib, name)(*a)  # noqa: E731
    halo0 = os.environ.get("CNNITMO_HALO") == "0"
    out = {"reachable": KC.reachable(q, halo0), "tested": KC.tested(q, halo0)}
    say(json.dumps(out))


def exact_names():
    sys.path.insert(0, ROOT)
    from tests import exact_cases as E
    from tests import kernel_cases as KC
    _, lib = load_lib()
    q = lambda name, *a: getattr(lib, name)(*a)  # noqa: E731
    halo0 = os.environ.get("CNNITMO_HALO") == "0"
    say(json.dumps({"tested": KC.tested(q, halo0), "launched": E.launched(q, halo0)}))


if __name__ == "__main__":
    {"sweep": sweep, "values": values, "launch": launch, "names": names, "exact_names": exact_names}[sys.argv[1]]()
