"""The walk cases of tests/walk_cases.py meet their conditions, on the library's host-only queries
(no GPU; 256 CUs, as the planners assume without a device), and every persistent kernel the
planners can choose in the documented domain has a walk case."""
import pytest

from tests import kernel_cases as KC
from tests import walk_cases as WC


@pytest.fixture(scope="module")
def q():
    import os
    from cnn_itmo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    _lib.load()
    return _lib.query


@pytest.mark.parametrize("case", list(WC.HALO), ids=lambda c: "-".join(str(v) for v in c[:6]))
def test_halo_case_walks(q, case):
    """(a), (b), (e): at least three tiles per stream, a row, a strip and an image step inside some
    range, partial last tile row and column, the name the case is there for."""
    sp = WC.check_halo(q, case)
    print(f"{case}: {sp['name']}, {sp['streams']} streams x {sp['nblocks']} blocks, {sp['tiles']} tiles, "
          f"{sp['per_stream']:.2f} per stream, {sp['idle']} workgroups idle")


def test_halo_set_has_idle_workgroups_and_every_form(q):
    """(a): some halo launch leaves workgroups without a stream (gs >= streams); the forms the
    name queries do not enumerate each have a case per dtype they exist in; the three store paths
    of the fused dgrad (kernel_cases.DGRAD_BN_BRANCH) are walked."""
    assert any(WC.halo_split(q, c)["idle"] for c in WC.HALO if c[0] == "fwd")
    assert any(WC.halo_split(q, c)["idle"] for c in WC.HALO if c[0] in ("dgrad", "dgrad_bn"))
    forms = {(c[0], c[1]) for c in WC.HALO}
    for op in WC.HALO_FORMS:
        for dt in ("bf16", "f32"):
            assert (op, dt) in forms or (op, dt) == ("fwd_cat", "f32"), f"no {dt} walk case of {op}"
    widths = {(c[1], WC.name_bn(WC.HALO[c])) for c in WC.HALO if c[0] == "fwd_nosum"}
    assert widths == {(dt, bn) for dt in ("bf16", "f32") for bn in (32, 64)}, widths
    assert set(WC.HALO_BRANCH) == set(KC.DGRAD_BN_BRANCH)
    seen = set()
    for (cin, cout, c0, c1, dt), w in WC.HALO_BRANCH.items():
        case = next(c for c in WC.HALO if c[0] == "dgrad_bn" and (c[1], c[3], c[4], c[5], c[6][:2]) == (dt, w, cin, cout, (c0, c1)))
        branch = KC.dgrad_bn_branch(WC.halo_name(q, case), dt, cin, c0, c1)
        assert branch == KC.DGRAD_BN_BRANCH[(cin, cout, c0, c1, dt)], (case, branch)
        seen.add(branch)
    assert seen == {"all", "mixed", "neither"}


@pytest.mark.parametrize("case", list(WC.TCONV), ids=lambda c: "-".join(str(v) for v in c))
def test_tconv_stream_case_walks(q, case):
    """(a), (d), (e): three tiles per group or none, idle groups, each step kind, a partial tile."""
    sp = WC.check_tconv(q, case)
    print(f"{case}: {sp['name']}, {sp['groups']} groups, {sp['ntiles']} tiles, {sp['per']} per group, "
          f"{sp['idle']} groups idle")


@pytest.mark.parametrize("case", list(WC.WGRAD), ids=lambda c: "-".join(str(v) for v in c))
def test_wgrad_halo_case_walks(q, case):
    """(a), (c), (e), for every occupancy the runtime may report."""
    sp = WC.check_wgrad(q, case)
    print(f"{case}: {sp['name']}, {sp['strips']} strips, {sp['rows']} rows; workgroups per CU -> (rows per range, ranges): "
          f"{ {o: (rp, len(r)) for o, (rp, r) in sp['plans'].items()} }")


def test_wgrad_halo_set(q):
    """(c): the R = 2 blocks walk an odd and an even row count; both strip widths have a partial
    last strip."""
    for occ, par in WC.wgrad_parities(q).items():
        assert par == {0, 1}, f"{occ} workgroups per CU: the two-rows-per-step blocks see row counts of parity {par} only"
    tws = {WC.wgrad_splits(q, c)["tw"] for c in WC.WGRAD}
    assert tws == {64, 128}


@pytest.mark.parametrize("case", list(WC.C3), ids=lambda c: "-".join(c))
def test_conv_c3_case_walks(q, case):
    sp = WC.check_c3(q, case)
    print(f"{case}: {sp['units']} units over at most {sp['groups']} workgroups, {sp['share']} each, {sp['pixels']} pixels")


def test_every_reachable_persistent_kernel_walks(q):
    """Coverage, as test_abi_and_host.test_dispatch_coverage: every halo_conv / tconv_stream /
    wgrad_halo name the planners give anywhere in the documented domain is the name of a walk case.
    No allow-list: a newly reachable persistent instantiation needs a walk."""
    reach = {k: v for k, v in KC.reachable(q).items() if k.startswith(WC.PERSISTENT)}
    walk = WC.walked(q)
    assert len(reach) >= 51, sorted(reach)
    print("kernel name | reached in the domain first at | walk case")
    for k in sorted(reach):
        print(f"{k} | {reach[k]} | {walk.get(k, 'NONE')}")
    missing = {k: reach[k] for k in reach if k not in walk}
    assert not missing, f"persistent kernels no walk case launches: {missing}"
