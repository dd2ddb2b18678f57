"""The packed-Shamir dispatch, restated once for the tests (CPU only; no product import beyond the schemes).

`gen_kernel` / `reveal_kernel` return the pretty name of the kernel instantiation that
`launch_packed_generate` / `launch_packed_reveal` (sda_amd/csrc/packed_gen.hip, packed_reveal.hip) launch
for a call, or "wide" for packed_wide.hip's workspace kernels.  The names are spelled as
scripts/code_objects.py demangles them, so tests/test_packed_matrix_plan.py can hold the plan of
tests/test_gpu_packed_matrix.py against the instantiations in the built library.

Restated here, each next to the line of the product it mirrors:
  gen_register_path, kLazyTruncMinP, make_gen_tables' big2 / big3 <= 4096 rule (the sign-bit flag), packed_gen_plan's
  pair-store (even B, 16-byte aligned out) rule and register / workspace choice, gen_launch_t's variant choice,
  packed_reveal_plan (reveal_plan.h): the reveal's workspace / register / detour paths, its 8/16/32/64/96 point
  buckets, its FULL / KU / STAGED choices and its lazy-only-at-the-threshold rule,
  wide_lanes, and which batches a launch logs for its fix-up kernel.
"""
import math

EXACT, CANONICAL = 0, 1                    # SDA_REVEAL_EXACT / SDA_REVEAL_CANONICAL

LAZY_TRUNC_MIN_P = 1 << 24                 # reveal_plan.h: kLazyTruncMinP
GEN_LOG_CAP = 1 << 16                      # kernels.h: kGenLogCap
REVEAL_MAX_POINTS = 96                     # reveal_plan.h: kRevealMaxPoints
REVEAL_KMAX = 64                           # reveal_plan.h: kRevealMaxK
SIGNBIT_MAX_BIG = 4096                     # packed_gen.hip: tab.flags
GEN_PARTS = {3: (2,), 9: (2, 4, 8), 27: (2, 4, 8, 16), 81: (2, 4, 8, 16, 32, 64)}    # Makefile: GEN_PARTS
REVEAL_PARTS = (8, 16, 32, 64, 96)         # Makefile: REVEAL_PARTS


def _b(x):
    return "true" if x else "false"


def gen_block(L):
    """packed_gen.hip: gen_block<L>() -- batches per workgroup."""
    return 256 if L <= 16 else (128 if L == 32 else 64)


def gen_register_path(L, N3, exact_nonlazy):
    """packed_gen.hip: gen_register_path."""
    return L <= 64 and N3 <= 81 and not (N3 == 81 and L >= 16 and exact_nonlazy)


def gen_bigs(sch):
    """(big2, big3) of make_gen_tables (packed_common.h): the largest ceil(p / w) over the non-unit radix-2
    twiddles, and over the two twiddles of the first radix-3 level."""
    p = sch.prime_modulus
    L, N3 = sch.secret_count + sch.privacy_threshold() + 1, sch.share_count + 1
    winv = pow(sch.omega_secrets, -1, p)
    big2 = 1
    ln = 4
    while ln <= L:                          # level len: omega = winv^(L / len), entries i = 1 .. len/2 - 1
        om = pow(winv, L // ln, p)
        for i in range(1, ln // 2):
            w = pow(om, i, p)
            if w > 1:
                big2 = max(big2, (p + w - 1) // w)
        ln *= 2
    w3 = pow(sch.omega_shares, N3 // 3, p)  # the len-3 level's omega
    big3 = 1
    for j in (1, 2):
        x = pow(w3, j, p)
        big3 = max(big3, (p + x - 1) // x)
    return big2, big3


def gen_signbit_flag(sch):
    """launch_packed_generate: tab.flags bit 0."""
    big2, big3 = gen_bigs(sch)
    return big2 <= SIGNBIT_MAX_BIG and big3 <= SIGNBIT_MAX_BIG


def gen_kernel(sch, B, out_mod16, mode, signbit_env=None):
    """The share-gen kernel of one launch: B batches per vector, output address mod 16, EXACT / CANONICAL,
    and the value of SDA_GEN_SIGNBIT (None: unset)."""
    p = sch.prime_modulus
    L, N3 = sch.secret_count + sch.privacy_threshold() + 1, sch.share_count + 1
    canon = mode == CANONICAL
    wide_store = B % 2 == 0 and out_mod16 % 16 == 0                 # packed_gen_plan: pair
    lazy_ok = p >= LAZY_TRUNC_MIN_P                                 # packed_gen_plan: lazy
    exact_nonlazy = not canon and not (wide_store and lazy_ok)
    if not gen_register_path(L, N3, exact_nonlazy):                 # packed_gen_plan: registers
        return "wide"
    assert L in GEN_PARTS.get(N3, ()), (L, N3)
    signbit = gen_signbit_flag(sch) and not (signbit_env is not None and str(signbit_env)[:1] == "0")   # GenLaunch::signbit
    if wide_store and not canon and lazy_ok:                        # gen_launch_t, from here on
        args = (True, False, True, signbit)
    elif wide_store:
        args = (True, canon, False, False)
    else:
        args = (False, canon, False, False)
    return f"packed_gen_kernel<{L}, {N3}, " + ", ".join(_b(a) for a in args) + ">"


def gen_kernel_is_lazy(name):
    return name.startswith("packed_gen_kernel<") and name.split(", ")[4] == "true"


def reveal_bucket(need):
    return next((mm for mm in REVEAL_PARTS if need <= mm), None)


def reveal_kernel(sch, n_idx, k, mode):
    """The reveal kernel of one launch from n_idx shares: packed_reveal_plan (sda_amd/csrc/reveal_plan.h), restated;
    tests/test_reveal_plan.py holds the two against each other on the CPU.  CANONICAL from more than 32 shares runs
    the exact kernel named here followed by launch_mod_canonical (reveal_takes_detour)."""
    p = sch.prime_modulus
    if n_idx + 1 > REVEAL_MAX_POINTS or k > REVEAL_KMAX:            # kRevealWorkspace
        return "wide"
    if reveal_takes_detour(n_idx, k, mode):                         # kRevealDetour: the plan's mode becomes EXACT
        mode = EXACT
    mm = reveal_bucket(n_idx + 1 if mode == EXACT else n_idx)       # the Lagrange kernels keep the shares only
    staged = k <= 16
    if mode == CANONICAL:
        return f"packed_reveal_canon_kernel<{mm}, {_b(staged)}>"
    if mm <= 16 and k <= 8:                                         # ku = 8
        # lazy only from exactly t + k shares (from more, the top Newton coefficients are 0 in every batch: the
        # lazy kernel's trap); then n_idx + 1 = k + t + 1 is a power of 2: 16 is FULL, 2 and 4 sit in the 8 bucket
        lazy = p >= LAZY_TRUNC_MIN_P and n_idx == k + sch.privacy_threshold()
        full = lazy and n_idx + 1 == mm
        lazy = lazy and (full or mm == 8)
        return f"packed_reveal_exact_kernel<{mm}, true, 8, {_b(lazy)}, {_b(full)}>"
    return f"packed_reveal_exact_kernel<{mm}, {_b(staged)}, 0, false, false>"


def reveal_takes_detour(n_idx, k, mode):
    """packed_reveal_plan: kRevealDetour -- the exact register kernels, then launch_mod_canonical."""
    return mode == CANONICAL and 32 < n_idx < REVEAL_MAX_POINTS and k <= REVEAL_KMAX


def reveal_kernel_is_lazy(name):
    return name.startswith("packed_reveal_exact_kernel<") and name.split(", ")[3] == "true"


def wide_lanes(total, words_per_lane):
    """packed_wide.hip: wide_lanes -- lanes in flight of the workspace kernels' grid-stride loop."""
    cap = (256 << 20) // (8 * words_per_lane)
    cap = min(max(cap, 4096), 65536)
    cap = (cap + 255) // 256 * 256
    want = (total + 255) // 256 * 256
    return min(want, cap)


def gen_fixup_count(kernel, planted, B):
    """Batches a share-gen launch logs, from the set of out-of-range batches {(vec, b)}: the register kernels
    log a batch when it or its store-pair partner b ^ 1 (if live) is out of range; the workspace kernels log
    nothing.  (The lazy kernels add their traps: gen_kernel_is_lazy.)"""
    if kernel == "wide":
        return 0
    logged = set()
    for vec, b in planted:
        assert 0 <= b < B
        logged.add((vec, b))
        if (b ^ 1) < B:
            logged.add((vec, b ^ 1))
    return len(logged)


def reveal_fixup_count(kernel, planted):
    """Batches a reveal launch logs (PackedRevealPlan::logged): the exact kernels log exactly the out-of-range batches; the canonical
    Lagrange kernels reduce raw shares in the lane and the workspace kernel takes any i64 -- neither logs."""
    return len(set(planted)) if kernel.startswith("packed_reveal_exact_kernel<") else 0


# ---------------------------------------------------------------------------------------------- number theory
def is_prime(n):
    """Deterministic Miller-Rabin for n < 3.3e9 (bases 2, 3, 5, 7)."""
    if n < 2:
        return False
    for q in (2, 3, 5, 7, 11, 13):
        if n % q == 0:
            return n == q
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for a in (2, 3, 5, 7):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def prime_below(L, N3, below):
    """The largest prime p = 1 mod lcm(L, N3) below `below`."""
    step = L * N3 // math.gcd(L, N3)
    c = (below - 2) // step
    while not is_prime(c * step + 1):
        c -= 1
    return c * step + 1


def roots(p, L, N3):
    """Roots of unity of order L and N3 mod p, from the smallest generator."""
    fac, x, d = set(), p - 1, 2
    while d * d <= x:
        while x % d == 0:
            fac.add(d)
            x //= d
        d += 1
    if x > 1:
        fac.add(x)
    g = next(g for g in range(2, p) if all(pow(g, (p - 1) // q, p) != 1 for q in fac))
    return pow(g, (p - 1) // L, p), pow(g, (p - 1) // N3, p)
