"""Integer model of the multilinear KZG commitment (PST13), written from the definitions with Python integers only: the
specification of csrc/mlpcs.hip and commitment/polynomial/mkzg.py, which are compared with it by ==.

A polynomial in m variables is the list of its 2^m values over {0,1}^m; variable 0 is the least significant bit of the list
index and point[i] goes to variable i.  Group elements appear as their discrete logarithms: a commitment is a scalar s standing
for s G."""


def eq_basis(point, p):
    """[eq(point; b) for b < 2^len(point)], eq(point; b) = prod_t (bit t of b ? point[t] : 1 - point[t])"""
    out = [1]
    for x in point:                       # variable t becomes bit t: the new bit is the most significant one so far
        out = [v * (1 - x) % p for v in out] + [v * x % p for v in out]
    return out


def evaluate(table, point, p):
    """the multilinear extension of `table` at `point`, from the definition: sum_b table[b] eq(point; b)"""
    assert len(table) == 1 << len(point)
    return sum(v * e for v, e in zip(table, eq_basis(point, p))) % p


def quotient_chain(table, point, p):
    """([q_0, .., q_(m-1)], v): q_k[b] = f_k[2b+1] - f_k[2b], f_(k+1)[b] = f_k[2b] + point[k] q_k[b], f_0 = table, v = f_m[0]"""
    assert len(table) == 1 << len(point)
    f, levels = [v % p for v in table], []
    for z in point:
        q = [(f[2 * b + 1] - f[2 * b]) % p for b in range(len(f) // 2)]
        f = [(f[2 * b] + z * q[b]) % p for b in range(len(q))]
        levels.append(q)
    return levels, f[0]


def level_offset(m, k):
    """where level k starts in the buffer of all 2^m - 1 quotient entries (level 0 first); level k has 2^(m-1-k) entries"""
    return (1 << m) - (1 << (m - k))


def flat_quotients(table, point, p):
    """the buffer the kernel fills: every level one after the other, and the evaluation"""
    levels, v = quotient_chain(table, point, p)
    flat = [x for q in levels for x in q]
    m = len(point)
    assert len(flat) == (1 << m) - 1 and all(level_offset(m, k) == sum(len(q) for q in levels[:k]) for k in range(m))
    return flat, v


# ---- the scheme in the exponent: tau = (tau_0 .. tau_(n-1)), a polynomial of m <= n variables uses tau_(n-m) onward ----
def commit(table, tau, p):
    """log of C = sum_b table[b] level_(n-m)[b] = f(tau_(n-m) .. tau_(n-1))"""
    m = len(table).bit_length() - 1
    return evaluate(table, tau[len(tau) - m:], p)


def open_(table, point, tau, p):
    """([log of Q_k], v): Q_k = sum_b q_k[b] level_(n-m+k+1)[b] = q_k(tau_(n-m+k+1) ..)"""
    m = len(point)
    levels, v = quotient_chain(table, point, p)
    first = len(tau) - m
    return [evaluate(q, tau[first + k + 1:], p) for k, q in enumerate(levels)], v


def identity_holds(table, point, at, p):
    """f(at) - f(point) == sum_k (at_k - point_k) q_k(at_(k+1) ..): what the pairing check tests at at = the trapdoor"""
    levels, v = quotient_chain(table, point, p)
    rhs = sum((at[k] - point[k]) * evaluate(q, at[k + 1:], p) for k, q in enumerate(levels))
    return (evaluate(table, at, p) - v - rhs) % p == 0


def combine(tables, rho, p):
    """sum_i rho^i f_i, entry by entry"""
    out, power = [0] * len(tables[0]), 1
    for t in tables:
        out = [(a + power * b) % p for a, b in zip(out, t)]
        power = power * rho % p
    return out


def combine_scalars(values, rho, p):
    return sum(pow(rho, i, p) * v for i, v in enumerate(values)) % p
