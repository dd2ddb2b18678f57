"""CPU: the plan of tests/test_gpu_packed_matrix.py against the packed-Shamir instantiations in the built
library (scripts/code_objects.py, as tests/test_kernel_resources.py reads them).

Every packed_gen_kernel / packed_reveal_exact_kernel / packed_reveal_canon_kernel instantiation that ships must
be the kernel tests/packed_dispatch.py predicts for at least one planned case, and no case may predict a name
the library lacks: a new instantiation fails here until a case of the matrix claims it.
"""
import importlib.util
import os

import pytest

from sda_amd import engine as E
from tests import packed_dispatch as PD
from tests import packed_matrix_cases as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("code_objects", os.path.join(ROOT, "scripts", "code_objects.py"))
CO = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(CO)

FAMILIES = ("packed_gen_kernel<", "packed_reveal_exact_kernel<", "packed_reveal_canon_kernel<")


@pytest.fixture(scope="module")
def shipped():
    if not os.path.exists(E.LIB_PATH):
        pytest.fail(f"{E.LIB_PATH} is not built (run __graft_entry__.build())")
    names = {k["pretty"] for k in CO.kernels(E.LIB_PATH) if k["pretty"].startswith(FAMILIES)}
    assert len(names) >= 90, "the fat binary parser found too few packed kernels"
    return names


def _planned():
    return {c.kernel for c in PM.GEN_CASES + PM.REVEAL_CASES} - {"wide"}


def test_every_shipped_instantiation_is_claimed_by_a_case(shipped):
    unclaimed = sorted(shipped - _planned())
    assert not unclaimed, f"instantiations no case of the matrix runs: {unclaimed}"


def test_no_case_predicts_a_kernel_the_library_lacks(shipped):
    invented = sorted(_planned() - shipped)
    assert not invented, f"predicted kernels missing from the library: {invented}"


def test_small_root_schemes_reach_the_lazy_kernel_without_sign_bits():
    """p = a^2 + 1 (omega_secrets^-1 = a) and p = a^2 + a + 1 (cube roots a, a^2): big2 resp. big3 is about
    sqrt(p) > 4096, so the default dispatch picks <L, N3, true, false, true, SIGNBIT = false>."""
    assert len(PM.SMALL_ROOT_SCHEMES) == 2
    for sch, side in zip(PM.SMALL_ROOT_SCHEMES, (0, 1)):
        assert sch.prime_modulus >= PD.LAZY_TRUNC_MIN_P
        assert PD.gen_bigs(sch)[side] > PD.SIGNBIT_MAX_BIG
        L, N3 = sch.secret_count + sch.privacy_threshold() + 1, sch.share_count + 1
        assert PD.gen_kernel(sch, PM.B_EVEN, 0, PD.EXACT) == f"packed_gen_kernel<{L}, {N3}, true, false, true, false>"
        assert pow(sch.omega_secrets, L, sch.prime_modulus) == 1 and pow(sch.omega_secrets, L // 2, sch.prime_modulus) != 1
        assert pow(sch.omega_shares, N3, sch.prime_modulus) == 1 and pow(sch.omega_shares, N3 // 3, sch.prime_modulus) != 1


def test_plan_shapes():
    """What the matrix relies on: 14 (L, N3) pairs with two primes each, D odd with a padded tail batch, grids
    that are no multiple of 8, and at least two (k, t) splits per L."""
    pairs = {}
    for c in PM.GEN_CASES[:-len(PM.SMALL_ROOT_SCHEMES)]:
        s = c.sch
        L, N3 = s.secret_count + s.privacy_threshold() + 1, s.share_count + 1
        pairs.setdefault((L, N3), set()).add(s.prime_modulus)
        D = PM.dimension(c.B, s.secret_count)
        assert (D + s.secret_count - 1) // s.secret_count == c.B
        if s.secret_count > 1:
            assert D % 2 == 1 and D % s.secret_count != 0
        tiles = -(-c.B // PD.gen_block(L))
        assert tiles >= 3 and (tiles * PM.V) % 8 != 0 and c.B % PD.gen_block(L) != 0
    assert len(pairs) == 14
    for ps in pairs.values():
        big, small = max(ps), min(ps)
        assert len(ps) == 2 and (1 << 30) < big < (1 << 31) and (1 << 16) <= small < (1 << 24)
    splits = {}
    for c in PM.GEN_CASES:
        s = c.sch
        splits.setdefault(s.secret_count + s.privacy_threshold() + 1, set()).add(s.secret_count)
    assert all(len(ks) >= 2 for L, ks in splits.items() if L > 2), splits
    assert 1 in splits[2] and any(k & (k - 1) for ks in splits.values() for k in ks)


def test_wide_lane_caps():
    assert PD.wide_lanes(10, 145) == 256
    assert PD.wide_lanes(3 * 21847, 64 + 81) == 65536
    assert PD.wide_lanes(1 << 20, 1241) == 27136
