"""CPU: the partial rounds of Poseidon as an order-3 recurrence on the S-box lane, restated in plain Python from the
plain constants (the oracle's round constants and MDS) and run against the oracle's permutation.  Independent of the
C++ table code (csrc/imt_params.cpp): the coefficients are derived here from the MDS alone.

In the plain form each partial round is s <- M (s + c_r + e0 (z_r - x_r)) with x_r the lane-0 S-box input and
z_r = x_r^5.  With M^3 = a2 M^2 + a1 M + a0 I (Cayley-Hamilton) and y_r = x_r - c_r,0 (lane 0 of the state):

    y_r+3 = (a2 - b0) y_r+2 + (a1 - b1) y_r+1 + a0 z_r + b1 z_r+1 + b0 z_r+2 + K_r,   b0 = M00, b1 = (M^2)00 - a2 M00

The device schedule holds the S-box input as x_r = lam_r (w_r + k_r) with lam_r+1 = b0 lam_r^5, so that z_r+2 enters
each step with coefficient 1.  The functions below mirror that schedule step by step on field elements."""
import ctypes
import random

from oracle_lib import P


def inv(x):
    return pow(x, P - 2, P)


def matmul(a, b):
    return [[sum(a[i][k] * b[k][j] for k in range(3)) % P for j in range(3)] for i in range(3)]


def matvec(m, v):
    return [sum(m[i][k] * v[k] for k in range(3)) % P for i in range(3)]


def plain_constants(oracle):
    rc = ctypes.create_string_buffer(195 * 32)
    mds = ctypes.create_string_buffer(9 * 32)
    oracle.lib.orc_poseidon_params(rc, mds)
    ints = lambda buf, n: [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]
    r = ints(rc, 195)
    m = ints(mds, 9)
    return [r[3 * i:3 * i + 3] for i in range(65)], [m[0:3], m[3:6], m[6:9]]


def derive(rc, M, lam0):
    """Coefficients of the recurrence schedule: per-round (C0, C1, C2, C3) on (w_r, w_r-1, z_r-2, z_r-1) (z_r enters
    with coefficient 1), S-box-input constants k_r, the entry functionals and the exit map."""
    M2 = matmul(M, M)
    a2 = (M[0][0] + M[1][1] + M[2][2]) % P
    minors = sum(M[i][i] * M[j][j] - M[i][j] * M[j][i] for i, j in ((0, 1), (0, 2), (1, 2)))
    det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
           + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0])) % P
    a1, a0 = (-minors) % P, det
    M3 = matmul(M2, M)
    for i in range(3):                                   # Cayley-Hamilton, as a check of a0, a1, a2
        for j in range(3):
            assert M3[i][j] == (a2 * M2[i][j] + a1 * M[i][j] + a0 * (i == j)) % P
    b0, b1 = M[0][0], (M2[0][0] - a2 * M[0][0]) % P
    c = rc[4:61]                                         # the partial rounds' constants, all three lanes
    N = [[(M2[i][j] - a2 * M[i][j]) % P for j in range(3)] for i in range(3)]
    K = [(matvec(N, c[p + 1])[0] - b1 * c[p + 1][0] + matvec(M, c[p + 2])[0] - b0 * c[p + 2][0]) % P for p in range(55)]
    lam = [lam0]
    for r in range(57):
        lam.append(b0 * pow(lam[-1], 5, P) % P)
    l5 = [pow(x, 5, P) for x in lam]
    # y_r = lam_r w_r + off_r
    off = [0, (M[0][1] * c[0][1] + M[0][2] * c[0][2]) % P]
    off.append((M2[0][1] * c[0][1] + M2[0][2] * c[0][2] + M[0][1] * c[1][1] + M[0][2] * c[1][2] - b0 * off[1]) % P)
    for r in range(2, 57):
        off.append(((a2 - b0) * off[r] + (a1 - b1) * off[r - 1] + K[r - 2]) % P)
    k = [(off[r] + c[r][0]) * inv(lam[r]) % P for r in range(57)]
    C = [(0, 1, 0, 0),
         ((-b0) * lam[1] * inv(lam[2]) % P, 0, 1, M2[0][0] * l5[0] * inv(lam[2]) % P)]
    for r in range(2, 57):
        li = inv(lam[r + 1])
        C.append(((a2 - b0) * lam[r] * li % P, (a1 - b1) * lam[r - 1] * li % P, a0 * l5[r - 2] * li % P,
                  b1 * l5[r - 1] * li % P))
    # entry: full round 3's rows 1 and 2 become the functionals of lanes 1, 2 that y_1 and y_2 need
    L1 = [(M[0][1] * M[1][j] + M[0][2] * M[2][j]) * inv(lam[1]) % P for j in range(3)]
    L2 = [(M2[0][1] * M[1][j] + M2[0][2] * M[2][j]) * inv(lam[2]) % P for j in range(3)]
    L0 = [M[0][j] * inv(lam[0]) % P for j in range(3)]
    # exit: the state after round 56 from (y_57, y_56, z_55, z_56); eta spans the left kernel of M's columns 1, 2
    col = lambda j: [M[i][j] for i in range(3)]
    u, v = col(1), col(2)
    eta = [(u[1] * v[2] - u[2] * v[1]) % P, (u[2] * v[0] - u[0] * v[2]) % P, (u[0] * v[1] - u[1] * v[0]) % P]
    g = [[M[0][1], M[0][2]], [eta[1], eta[2]]]
    gdet = (g[0][0] * g[1][1] - g[0][1] * g[1][0]) % P
    assert gdet != 0
    gi = [[g[1][1] * inv(gdet) % P, -g[0][1] * inv(gdet) % P], [-g[1][0] * inv(gdet) % P, g[0][0] * inv(gdet) % P]]
    eta_c = sum(e * x for e, x in zip(eta, c[56])) % P
    eta_m0 = sum(eta[i] * M[i][0] for i in range(3)) % P

    def exit_state(y57, y56, z55, z56):
        r1 = (y57 - M[0][0] * z56) % P
        r2 = (eta_c + eta_m0 * z55 - eta[0] * (y56 + c[56][0])) % P
        v1 = (gi[0][0] * r1 + gi[0][1] * r2) % P
        v2 = (gi[1][0] * r1 + gi[1][1] * r2) % P
        return matvec(M, [z56, v1, v2])

    return dict(lam=lam, l5=l5, off=off, k=k, C=C, L=(L0, L1, L2), exit_state=exit_state, a0=a0)


def permute_recurrence(rc, M, d, s):
    sbox = lambda x: pow(x, 5, P)
    s = list(s)
    for r in range(4):
        s = [sbox((s[i] + rc[r][i]) % P) for i in range(3)]
        if r < 3:
            s = matvec(M, s)
    L0, L1, L2 = d["L"]
    # window before round r: A = w_r, B = w_r-1, Z3 = z_r-2, Z2 = z_r-1 (scaled); round 0 is seeded with the
    # entry functionals so that every round runs the same body
    A = sum(L0[j] * s[j] for j in range(3)) % P
    B = sum(L1[j] * s[j] for j in range(3)) % P
    Z3, Z2 = 0, sum(L2[j] * s[j] for j in range(3)) % P
    for r in range(57):
        Z = sbox((A + d["k"][r]) % P)
        c0, c1, c2, c3 = d["C"][r]
        W = (c0 * A + c1 * B + c2 * Z3 + c3 * Z2 + Z) % P
        A, B, Z3, Z2 = W, A, Z2, Z
    lam, l5, off = d["lam"], d["l5"], d["off"]
    y57, y56 = (lam[57] * A + off[57]) % P, (lam[56] * B + off[56]) % P
    s = d["exit_state"](y57, y56, l5[55] * Z3 % P, l5[56] * Z2 % P)
    for r in range(61, 65):
        s = matvec(M, [sbox((s[i] + rc[r][i]) % P) for i in range(3)])
    return s


def test_recurrence_restatement_matches_oracle(oracle):
    rc, M = plain_constants(oracle)
    rng = random.Random(0x3EC0)
    for lam0 in (1, 7, rng.randrange(1, P)):
        d = derive(rc, M, lam0)
        states = [[0, 0, 0], [P - 1] * 3, [1, 2, 3]] + [[rng.randrange(P) for _ in range(3)] for _ in range(40)]
        for st in states:
            assert permute_recurrence(rc, M, d, st) == oracle.permute(st), (lam0, st)


def test_recurrence_drops_the_oldest_lane0_value(oracle):
    """The a0 y_r term cancels: y_r+3 depends on the lane-0 values only through y_r+2 and y_r+1.  The plain partial
    rounds are run from three random states, and the residual y_r+3 - (the recurrence's five terms) must be the same
    constant sequence K_r for each: it does not depend on the state."""
    rc, M = plain_constants(oracle)
    d = derive(rc, M, 1)
    assert d["a0"] != 0
    M2 = matmul(M, M)
    a2 = (M[0][0] + M[1][1] + M[2][2]) % P
    b0, b1 = M[0][0], (M2[0][0] - a2 * M[0][0]) % P
    # run the plain partial rounds and record y, z; the recurrence residual must be the same constant for any state
    rng = random.Random(7)
    residuals = []
    for _ in range(3):
        s = [rng.randrange(P) for _ in range(3)]
        ys, zs = [], []
        for r in range(4, 61):
            s = [(s[i] + rc[r][i]) % P for i in range(3)]
            ys.append((s[0] - rc[r][0]) % P)
            s[0] = pow(s[0], 5, P)
            zs.append(s[0])
            s = matvec(M, s)
        ys.append(s[0])
        minors = sum(M[i][i] * M[j][j] - M[i][j] * M[j][i] for i, j in ((0, 1), (0, 2), (1, 2)))
        a1 = (-minors) % P
        residuals.append([(ys[r + 3] - (a2 - b0) * ys[r + 2] - (a1 - b1) * ys[r + 1] - d["a0"] * zs[r] - b1 * zs[r + 1]
                           - b0 * zs[r + 2]) % P for r in range(55)])
    assert residuals[0] == residuals[1] == residuals[2]
