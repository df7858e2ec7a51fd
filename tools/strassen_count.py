"""Flop count of the fused Cholesky + inverse recursion (potrf.hip) with the structured splits and
Strassen routing: algorithmic flops per class, executed flops and operand-sum bytes."""
import sys
NB, NBI = 128, 512


def split_point(n):
    nb = (n + NB - 1) // NB
    return NB * (nb // 2)


class C:
    def __init__(s, min_dim, levels):
        s.min, s.lv = min_dim, levels
        s.classical = 0.0   # flops as the classical recursion counts them
        s.executed = 0.0    # flops of the launches made
        s.plain_big = 0.0   # classical flops of the Strassen-eligible plain products
        s.add_bytes = 0.0
        s.adds = 0

    def ok(s, m, n, k):
        return s.lv > 0 and all(d % 256 == 0 and d >= s.min for d in (m, n, k))

    def strassen(s, m, n, k, lv):
        if lv <= 0 or not s.ok(m, n, k):
            s.executed += 2.0 * m * n * k
            return
        m2, n2, k2 = m // 2, n // 2, k // 2
        s.add_bytes += 24.0 * (5 * m2 * k2 + 5 * k2 * n2)
        s.adds += 10
        for _ in range(7):
            s.strassen(m2, n2, k2, lv - 1)

    def plain(s, m, n, k):
        s.classical += 2.0 * m * n * k
        if s.ok(m, n, k):
            s.plain_big += 2.0 * m * n * k
            s.strassen(m, n, k, s.lv)
        else:
            s.executed += 2.0 * m * n * k

    def struct(s, fl):
        s.classical += fl
        s.executed += fl

    def syrk(s, n, k):
        h = n // 2
        if n % 2 == 0 and s.ok(h, h, k):
            s.syrk(h, k); s.plain(h, h, k); s.syrk(h, k)
        else:
            s.struct(k * n * (n + 1.0))

    def trmm_b(s, m, n):
        h = n // 2
        if n % 2 == 0 and s.ok(m, h, h):
            s.trmm_b(m, h); s.plain(m, h, h); s.trmm_b(m, h)
        else:
            s.struct(1.0 * m * n * n)

    def trmm_a(s, m, n):
        h = m // 2
        if m % 2 == 0 and s.ok(h, n, h):
            s.trmm_a(h, n); s.trmm_a(h, n); s.plain(h, n, h)
        else:
            s.struct(1.0 * m * n * m)

    def trsm(s, m, nL):
        if nL <= NBI:
            s.struct(1.0 * m * nL * nL)
            return
        a = split_point(nL); b = nL - a
        s.trsm(m, a); s.plain(m, b, a); s.trsm(m, b)

    def potrf(s, n):
        if n <= NBI:
            s.struct(n ** 3 / 3.0 + n ** 3 / 3.0)  # block factor + its inverse
            return
        n1 = split_point(n); n2 = n - n1
        s.potrf(n1); s.trsm(n2, n1); s.syrk(n2, n1); s.potrf(n2)

    def trtri(s, n):
        if n <= NBI:
            return
        n1 = split_point(n); n2 = n - n1
        s.trtri(n1); s.trtri(n2); s.trmm_b(n2, n1); s.trmm_a(n2, n1)


N = int(sys.argv[1]) if len(sys.argv) > 1 else 65536
for md, lv in ((8192, 0), (8192, 1), (8192, 2), (16384, 1), (16384, 2)):
    c = C(md, lv)
    c.potrf(N); c.trtri(N)
    print(f"min_dim {md:6d} levels {lv}: classical {c.classical:.4e} (2N^3/3 = {2 * N ** 3 / 3:.4e}) "
          f"eligible share {c.plain_big / c.classical:.3f} executed x{c.executed / c.classical:.4f} "
          f"= {c.executed:.4e}; {c.adds} operand sums, {c.add_bytes / 1e9:.0f} GB")
