"""The plan of tests/test_gpu_packed_matrix.py: every case, with the kernel tests/packed_dispatch.py predicts
for it, built on the CPU at import (no GPU, no product import beyond the schemes).

tests/test_packed_matrix_plan.py holds the plan against the instantiations in the built library: each
packed_gen_kernel / packed_reveal_{exact,canon}_kernel instantiation must be some case's predicted kernel.
"""
from dataclasses import dataclass
from typing import Optional

from sda_amd import schemes as S
from tests import packed_dispatch as PD

V = 3                      # vectors per launch: blockIdx.y > 0, a grid that is no multiple of 8
B_EVEN, B_ODD = 550, 549   # two or more full tiles and a ragged one at every workgroup size (256, 128, 64)

# (k, t) splits per L = k + t + 1, taken in turn over the cases of that L
SPLITS = {2: [(1, 0)], 4: [(3, 0), (1, 2), (2, 1)], 8: [(3, 4), (7, 0), (5, 2)], 16: [(8, 7), (11, 4), (15, 0)],
          32: [(17, 14), (13, 18)], 64: [(33, 30), (52, 11)]}


def scheme_for(k, t, n, below=1 << 31):
    L, N3 = k + t + 1, n + 1
    p = PD.prime_below(L, N3, below)
    ws, wn = PD.roots(p, L, N3)
    return S.PackedShamir(k, n, t, p, ws, wn)


def sid(s):
    return f"k{s.secret_count}t{s.privacy_threshold()}n{s.share_count}p{s.prime_modulus}"


def dimension(B, k):
    """D = B k - r, odd, 0 < r < k wherever k > 1: a zero-padded tail batch, and vector 1 starts 8 bytes off
    a 16-byte boundary."""
    if k == 1:
        return B
    return next(B * k - r for r in range(1, k) if (B * k - r) % 2 == 1)


@dataclass(frozen=True)
class GenCase:
    name: str
    sch: S.PackedShamir
    B: int
    out_offset: int            # bytes added to a 16-byte aligned output pointer
    mode: int
    signbit_env: Optional[str]
    kernel: str                # predicted

    @property
    def id(self):
        return f"{sid(self.sch)}-{self.name}"


@dataclass(frozen=True)
class RevealCase:
    sch: S.PackedShamir
    n_idx: int
    mode: int
    B: int
    kernel: str                # predicted (CANONICAL past 32 shares: the exact kernel of the detour)

    @property
    def id(self):
        return f"{sid(self.sch)}-from{self.n_idx}-{'canon' if self.mode else 'exact'}-B{self.B}"


def _gen_variants(sch, big):
    v = [("exact", B_EVEN, 0, PD.EXACT, None)]
    if big:
        v.append(("exact-signbit0", B_EVEN, 0, PD.EXACT, "0"))
    v += [("exact-oddB", B_ODD, 0, PD.EXACT, None), ("exact-off8", B_EVEN, 8, PD.EXACT, None),
          ("canon", B_EVEN, 0, PD.CANONICAL, None), ("canon-oddB", B_ODD, 0, PD.CANONICAL, None)]
    return [GenCase(name, sch, B, off, mode, env, PD.gen_kernel(sch, B, off, mode, env))
            for name, B, off, mode, env in v]


def _small_root_schemes():
    """Schemes that reach the lazy exact kernel WITHOUT sign bits with no knob set (big2 or big3 > 4096):
    p = a^2 + 1 with L = 4, whose order-4 roots are +-a (omega_secrets^-1 = a: big2 = ceil(p / a) ~ a), and
    p = a^2 + a + 1, whose cube roots of unity are a and a^2 = p - a - 1 (big3 ~ a)."""
    out = []
    a = 46340 // 18 * 18                       # 4 * 9 | a^2
    while not PD.is_prime(a * a + 1):
        a -= 18
    p = a * a + 1
    _, wn = PD.roots(p, 4, 9)
    out.append(S.PackedShamir(2, 8, 1, p, p - a, wn))
    a = 46339
    while not (PD.is_prime(a * a + a + 1) and a * (a + 1) % (8 * 27) == 0 and a * a + a + 1 < (1 << 31)):
        a -= 1
    p = a * a + a + 1
    ws, wn = PD.roots(p, 8, 27)
    out.append(S.PackedShamir(5, 26, 2, p, ws, wn))
    return out


def _build_gen():
    cases, turn = [], {L: 0 for L in SPLITS}
    for N3, Ls in PD.GEN_PARTS.items():
        for L in Ls:
            for below in (1 << 31, 1 << 24):
                k, t = SPLITS[L][turn[L] % len(SPLITS[L])]
                turn[L] += 1
                sch = scheme_for(k, t, N3 - 1, below)
                assert below == 1 << 31 or sch.prime_modulus >= 1 << 16
                cases += _gen_variants(sch, below == 1 << 31)
    return cases


SMALL_ROOT_SCHEMES = _small_root_schemes()
GEN_CASES = _build_gen() + [GenCase("exact-default-nosignbit", s, B_EVEN, 0, PD.EXACT, None,
                                    PD.gen_kernel(s, B_EVEN, 0, PD.EXACT, None)) for s in SMALL_ROOT_SCHEMES]


def _build_reveal():
    big, small = 1 << 31, 1 << 24
    rows = [  # (k, t, n, below, n_idx, mode)
        (3, 4, 8, big, 7, PD.EXACT),          # <8, KU 8, lazy, FULL>
        (1, 2, 8, big, 3, PD.EXACT),          # <8, KU 8, lazy>, 4 of 8 points
        (1, 0, 2, big, 1, PD.EXACT),          # <8, KU 8, lazy>, 2 points
        (1, 2, 8, big, 5, PD.EXACT),          # <8, KU 8, non-lazy>: past t + k shares the lazy kernel would trap
        (3, 4, 8, small, 7, PD.EXACT),        # <8, KU 8, non-lazy>
        (8, 7, 26, big, 15, PD.EXACT),        # <16, KU 8, lazy, FULL>
        (3, 4, 26, big, 12, PD.EXACT),        # <16, KU 8, non-lazy>: more than t + k shares
        (8, 7, 26, small, 15, PD.EXACT),      # <16, KU 8, non-lazy>
        (5, 2, 26, small, 9, PD.EXACT),       # <16, KU 8, non-lazy>, not full
        (11, 4, 26, big, 15, PD.EXACT),       # <16, staged, KU 0>
        (8, 7, 26, big, 21, PD.EXACT),        # <32, staged>
        (11, 4, 26, small, 26, PD.EXACT),     # <32, staged>, 8 < k
        (17, 14, 80, big, 31, PD.EXACT),      # <32, unstaged>
        (8, 7, 80, big, 40, PD.EXACT),        # <64, staged>
        (20, 11, 80, big, 50, PD.EXACT),      # <64, unstaged>
        (8, 7, 80, small, 80, PD.EXACT),      # <96, staged>
        (5, 2, 242, big, 95, PD.EXACT),       # <96, staged>, the last point count of the register kernels
        (33, 30, 80, big, 80, PD.EXACT),      # <96, unstaged>
        (3, 4, 8, big, 8, PD.CANONICAL),      # canon <8, staged>
        (1, 0, 8, small, 3, PD.CANONICAL),    # canon <8, staged>, few shares
        (8, 7, 26, big, 16, PD.CANONICAL),    # canon <16, staged>
        (11, 4, 26, small, 15, PD.CANONICAL),  # canon <16, staged>, 8 < k
        (8, 7, 80, big, 32, PD.CANONICAL),    # canon <32, staged>
        (17, 14, 80, big, 31, PD.CANONICAL),  # canon <32, unstaged>
        (8, 7, 80, big, 40, PD.CANONICAL),    # detour: exact <64> + launch_mod_canonical
        (20, 11, 80, small, 80, PD.CANONICAL),  # detour: exact <96, unstaged>
    ]
    cases = []
    for i, (k, t, n, below, n_idx, mode) in enumerate(rows):
        sch = scheme_for(k, t, n, below)
        assert t + k <= n_idx <= n
        B = B_ODD if i % 2 or k == 1 else B_EVEN          # k = 1: D = B, and D is odd in every case
        cases.append(RevealCase(sch, n_idx, mode, B, PD.reveal_kernel(sch, n_idx, k, mode)))
    return cases


REVEAL_CASES = _build_reveal()


def xcd_gen_cases():
    """The rows whose kernels read SDA_XCD_ORDER (packed_gen.hip: L <= 16)."""
    return [c for c in GEN_CASES if c.sch.secret_count + c.sch.privacy_threshold() + 1 <= 16 and c.kernel != "wide"]


def xcd_reveal_cases():
    """packed_reveal.hip: the kernels of up to 16 points."""
    return [c for c in REVEAL_CASES if "_kernel<8," in c.kernel or "_kernel<16," in c.kernel]
