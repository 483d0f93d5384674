"""Lattice builders with the reference's edge ordering (benches/end_to_end.rs:8-30)."""


def one_d_periodic(l, j=1.0):
    return [((i, (i + 1) % l), j) for i in range(l)]


def two_d_periodic(l, jfun=None):
    """Site (i,j) -> j*l+i; all right bonds first, then all down bonds; default = the benches' Villain pattern."""
    idx = [(i, j) for i in range(l) for j in range(l)]
    f = lambda i, j: j * l + i
    if jfun is None:
        jfun = lambda i, j, d: -1.0 if d == 0 else (1.0 if i % 2 == 0 else -1.0)
    right = [((f(i, j), f((i + 1) % l, j)), jfun(i, j, 0)) for i, j in idx]
    down = [((f(i, j), f(i, (j + 1) % l)), jfun(i, j, 1)) for i, j in idx]
    return right + down


def two_d_ferro(l):
    return two_d_periodic(l, lambda i, j, d: -1.0)


def rect_periodic(lx, ly, jfun=None):
    """lx x ly periodic lattice with the ordering rule of two_d_periodic: site (i,j) -> j*lx+i, i < lx, j < ly, visited with i
    outermost; all right bonds first, then all down bonds (a side of length 1 or 2 gives self-loops or duplicate edges:
    callers keep both sides >= 3)."""
    idx = [(i, j) for i in range(lx) for j in range(ly)]
    f = lambda i, j: j * lx + i
    if jfun is None:
        jfun = lambda i, j, d: -1.0 if d == 0 else (1.0 if i % 2 == 0 else -1.0)
    right = [((f(i, j), f((i + 1) % lx, j)), jfun(i, j, 0)) for i, j in idx]
    down = [((f(i, j), f(i, (j + 1) % ly)), jfun(i, j, 1)) for i, j in idx]
    return right + down


def star(n, j=1.0):
    """Variable 0 joined to each of 1 .. n-1 (degree n - 1 at the centre, 1 everywhere else)."""
    return [((0, v), j) for v in range(1, n)]


def complete(n, j=1.0):
    """Every pair (a, b), a < b, in lexicographic order."""
    return [((a, b), j) for a in range(n) for b in range(a + 1, n)]


def split(edges):
    return [list(e) for e, _ in edges], [j for _, j in edges]


def cubic_periodic(l):
    """Periodic simple-cubic lattice, site (x,y,z) -> (z*l + y)*l + x, edges +x, +y, +z per site (J filled in by the caller)."""
    edges = []
    for z in range(l):
        for y in range(l):
            for x in range(l):
                a = (z * l + y) * l + x
                edges.append(((a, (z * l + y) * l + (x + 1) % l), 1.0))
                edges.append(((a, (z * l + (y + 1) % l) * l + x), 1.0))
                edges.append(((a, (((z + 1) % l) * l + y) * l + x), 1.0))
    return edges


def xxz_ring_interactions(n, t=1.0, jz=0.5, c=1.0, hx=0.3):
    """Generic-interaction test model on a ring of n sites (weights = matrix elements of -H_b + const, all >= 0):
    two-site bonds with hopping t (|01> <-> |10>), Ising part jz (favouring aligned spins) and constant c on the diagonal;
    one-site bonds hx*(sigma_x + 1).  Matrices in the reference's layout (index = out0 out1 in0 in1, qmc_runner.rs:666-679).
    Returns [(mat, vars), ...]."""
    import numpy as np
    ints = []
    for i in range(n):
        m = np.zeros(16)
        for s in range(4):  # s = (s0 s1), first variable most significant
            aligned = ((s >> 1) & 1) == (s & 1)
            m[(s << 2) | s] = c + (jz if aligned else 0.0)
        m[(0b01 << 2) | 0b10] = t
        m[(0b10 << 2) | 0b01] = t
        ints.append((m, (i, (i + 1) % n)))
    for i in range(n):
        ints.append((np.full(4, hx), (i,)))
    return ints


def exact_energy_from_interactions(n, ints, beta):
    """<H> at inverse temperature beta for H = -sum_b M_b (dense, n <= 10)."""
    import numpy as np
    dim = 1 << n
    H = np.zeros((dim, dim))
    for mat, vs in ints:
        k = len(vs)
        for s_in in range(dim):
            bits_in = [(s_in >> (n - 1 - v)) & 1 for v in vs]
            iin = 0
            for bbit in bits_in:
                iin = (iin << 1) | bbit
            for iout in range(1 << k):
                w = mat[(iout << k) | iin]
                if w == 0.0:
                    continue
                s_out = s_in
                for j, v in enumerate(vs):
                    ob = (iout >> (k - 1 - j)) & 1
                    s_out = (s_out & ~(1 << (n - 1 - v))) | (ob << (n - 1 - v))
                H[s_out, s_in] -= w
    ev = np.linalg.eigvalsh(H)
    wts = np.exp(-beta * (ev - ev.min()))
    return float((ev * wts).sum() / wts.sum())


# ---- the size ladder of tests/test_gpu_shape_edges.py: one model on each side of every gate of isingmc_create / run() ----
def chain(n, jfun):
    """Periodic chain of n >= 3 sites; two sites: one bond; one site: no edge at all."""
    if n == 1:
        return []
    if n == 2:
        return [((0, 1), jfun(0))]
    return [((i, (i + 1) % n), jfun(i)) for i in range(n)]


def uni_chain(i):   # uniform |J|, mixed signs
    return -1.0 if i % 3 == 0 else 1.0


def mix_chain(i):   # four magnitudes, mixed signs: the general bond table
    return (0.5 + 0.25 * (i % 4)) * (-1.0 if i % 3 == 0 else 1.0)


def uni_rect(i, j, d):
    return -1.0 if (i + 2 * j + d) % 3 == 0 else 1.0


def mix_rect(i, j, d):
    return (0.5 + 0.25 * ((i + j) % 4)) * (-1.0 if (i + 2 * j + d) % 3 == 0 else 1.0)


SMALL = [1, 2, 31, 32, 33, 63, 64, 65, 127, 129, 1023, 1025, 2047]
UNIFORM_CHAINS = SMALL + [4071, 4072, 4095, 4096, 4097, 8480, 8481, 11041, 11042, 12288, 12289]
UNIFORM_RECTS = [(31, 33), (45, 91), (64, 64), (17, 241), (64, 96), (65, 95)]
MIXED_CHAINS = [1, 2, 31, 33, 65, 129, 1025, 4095, 4096, 4097, 8481, 11041, 11042]
MIXED_RECTS = [(45, 91), (17, 241)]
# (name, edges, nvars, h)
LADDER = ([(f"chain{n}", chain(n, uni_chain), n, 0.0) for n in UNIFORM_CHAINS] +
          [(f"rect{x}x{y}", rect_periodic(x, y, uni_rect), x * y, 0.0) for x, y in UNIFORM_RECTS] +
          [(f"mixchain{n}", chain(n, mix_chain), n, 0.0) for n in MIXED_CHAINS] +
          [(f"mixrect{x}x{y}", rect_periodic(x, y, mix_rect), x * y, 0.0) for x, y in MIXED_RECTS] +
          [(f"chain{n}_long", chain(n, uni_chain), n, 0.2) for n in (1, 33, 1025, 4096, 11042)] +
          [("rect17x241_long", rect_periodic(17, 241, uni_rect), 4097, -0.15), ("mixchain4097_long", chain(4097, mix_chain), 4097, 0.2)])
LADDER_IDS = [c[0] for c in LADDER]
assert len(set(LADDER_IDS)) == len(LADDER)
