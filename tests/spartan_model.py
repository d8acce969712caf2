"""Integer model of Spartan (the NIZK variant) over R1CS, written from the definitions with Python integers only: the specification of
csrc/spartan.hip and zksnake_amd/spartan, which are compared with it by ==.

Conventions are those of mlpcs_model.py: a table of 2^m values, variable 0 is the least significant bit of the index, point[t]
goes to variable t.  Group elements appear as their discrete logarithms.  CHALLENGES ARE INPUTS: `ch` is a dict with
tau (s_x), rx (s_x), r_abc (3), ry (s); `kzg_tau` (h) is the trapdoor of the commitment.

An instance is a dict: A, B, C = lists of (row, col, value) triplets (repeats add), n_row, n_col, n_public, p."""

import mlpcs_model as M


def log2_ceil(n):
    return max(1, (n - 1).bit_length())


def sizes(inst):
    """(s_x, h, s): constraint variables, variables of the committed table, variables of z"""
    s_x = log2_ceil(inst["n_row"])
    h = log2_ceil(max(inst["n_col"] - inst["n_public"], inst["n_public"]))
    return s_x, h, h + 1


def column(j, n_public, h):
    """where wire j sits in z: private wires fill the low half from 0, public ones (the constant first) the high half"""
    return j - n_public if j >= n_public else (1 << h) + j


def tables(inst, public, private):
    """(w, z): the committed table of 2^h entries and the whole assignment of 2^s entries, zero padded"""
    _, h, s = sizes(inst)
    p, n_public = inst["p"], inst["n_public"]
    assert len(public) == n_public and len(private) == inst["n_col"] - n_public
    z = [0] * (1 << s)
    for j, v in enumerate(list(public) + list(private)):
        z[column(j, n_public, h)] = v % p
    return z[:1 << h], z


# ---- the merged three-matrix CSR and the two kernel contracts ---------------------------------------------------------------
def merged_csr(n_seg, mats):
    """mats: three lists of (segment, idx, value).  (ptr[3 n_seg + 1], idx, val): sub-segment 3 i + m holds matrix m's entries of
    segment i, in the order given"""
    buckets = [[] for _ in range(3 * n_seg)]
    for m, entries in enumerate(mats):
        for seg, i, v in entries:
            buckets[3 * seg + m].append((i, v))
    ptr, idx, val = [0], [], []
    for b in buckets:
        idx += [i for i, _ in b]
        val += [v for _, v in b]
        ptr.append(len(idx))
    return ptr, idx, val


def accumulate(ptr, idx, val, x, p):
    """acc[i][m] = sum val[k] x[idx[k]] over sub-segment 3 i + m, entry by entry"""
    n_seg = (len(ptr) - 1) // 3
    acc = [[0, 0, 0] for _ in range(n_seg)]
    for i in range(n_seg):
        for m in range(3):
            for k in range(ptr[3 * i + m], ptr[3 * i + m + 1]):
                acc[i][m] = (acc[i][m] + val[k] * x[idx[k]]) % p
    return acc


def products(ptr, idx, val, z, p):
    """zk_r1cs_products_dev: (az, bz, cz)"""
    acc = accumulate(ptr, idx, val, z, p)
    return tuple([a[m] for a in acc] for m in range(3))


def bind(ptr, idx, val, e, coeff, p):
    """zk_r1cs_bind_dev: out[y] = cA acc_A + cB acc_B + cC acc_C, the coefficients reduced on entry"""
    c = [v % p for v in coeff]
    return [(c[0] * a[0] + c[1] * a[1] + c[2] * a[2]) % p for a in accumulate(ptr, idx, val, e, p)]


def row_major(inst):
    """the merged CSR with constraints as segments and permuted columns as idx (2^s_x segments)"""
    s_x, h, _ = sizes(inst)
    n_public, p = inst["n_public"], inst["p"]
    return merged_csr(1 << s_x, [[(r, column(c, n_public, h), v % p) for r, c, v in inst[name]] for name in "ABC"])


def col_major(inst):
    """the merged CSR with permuted columns as segments and constraints as idx (2^s segments)"""
    _, h, s = sizes(inst)
    n_public, p = inst["n_public"], inst["p"]
    return merged_csr(1 << s, [[(column(c, n_public, h), r, v % p) for r, c, v in inst[name]] for name in "ABC"])


def dense(inst):
    """A, B, C as dense 2^s_x x 2^s matrices in the permuted layout"""
    s_x, h, s = sizes(inst)
    out = []
    for name in "ABC":
        m = [[0] * (1 << s) for _ in range(1 << s_x)]
        for r, c, v in inst[name]:
            y = column(c, inst["n_public"], h)
            m[r][y] = (m[r][y] + v) % inst["p"]
        out.append(m)
    return out


# ---- polynomials through small integer points -------------------------------------------------------------------------------
def interpolate(ys, p):
    """coefficients (lowest first) of the polynomial of degree < len(ys) through (t, ys[t])"""
    n = len(ys)
    out = [0] * n
    for j, y in enumerate(ys):
        num, den = [1], 1
        for m in range(n):
            if m != j:
                num = [(a - m * b) % p for a, b in zip([0] + num, num + [0])]
                den = den * (j - m) % p
        scale = y * pow(den, -1, p) % p
        for i, c in enumerate(num):
            out[i] = (out[i] + scale * c) % p
    return out


def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def eq_point(a, b, p):
    out = 1
    for x, y in zip(a, b):
        out = out * (x * y + (1 - x) * (1 - y)) % p
    return out


def bits(b, n):
    return [(b >> t) & 1 for t in range(n)]


# ---- the prover from the dense definition -------------------------------------------------------------------------------------
def rounds_dense(f, n_vars, degree, r, p):
    """the sumcheck messages of f (a function of a point of n_vars coordinates): round j is the polynomial in X of
    sum over x' in {0,1}^(n_vars-j-1) of f(r[:j], X, x'), sampled at 0 .. degree and interpolated"""
    out = []
    for j in range(n_vars):
        rest = n_vars - j - 1
        ys = [sum(f(list(r[:j]) + [t] + bits(b, rest)) for b in range(1 << rest)) % p for t in range(degree + 1)]
        out.append(interpolate(ys, p))
    return out


def prove_dense(inst, public, private, ch, kzg_tau):
    p = inst["p"]
    s_x, h, s = sizes(inst)
    w, z = tables(inst, public, private)
    A, B, C = dense(inst)
    az, bz, cz = ([sum(a * b for a, b in zip(row, z)) % p for row in m] for m in (A, B, C))
    tau, rx, (ra, rb, rc), ry = ch["tau"], ch["rx"], ch["r_abc"], ch["ry"]

    def outer(pt):
        return eq_point(tau, pt, p) * (M.evaluate(az, pt, p) * M.evaluate(bz, pt, p) - M.evaluate(cz, pt, p)) % p

    evals = tuple(M.evaluate(t, rx, p) for t in (az, bz, cz))
    ex = M.eq_basis(rx, p)
    m_r = [sum(ex[i] * (ra * A[i][y] + rb * B[i][y] + rc * C[i][y]) for i in range(1 << s_x)) % p for y in range(1 << s)]

    def inner(pt):
        return M.evaluate(m_r, pt, p) * M.evaluate(z, pt, p) % p

    quotients, v_w = M.open_(w, ry[:h], kzg_tau, p)
    return {"commitment": M.commit(w, kzg_tau, p), "outer": rounds_dense(outer, s_x, 3, rx, p), "evals": evals,
            "inner": rounds_dense(inner, s, 2, ry, p), "v_w": v_w, "opening": quotients}


# ---- the prover in linear time ------------------------------------------------------------------------------------------------
def fold(table, r, p):
    return [(table[2 * b] + r * (table[2 * b + 1] - table[2 * b])) % p for b in range(len(table) // 2)]


def rounds_linear(tabs, terms, degree, r, p):
    """the sumcheck messages of sum_t c_t prod_(i in which_t) tabs[i], by folding the tables one variable per round"""
    out = []
    for j in range(len(r)):
        ys = []
        for t in range(degree + 1):
            at = [[(tb[2 * b] + t * (tb[2 * b + 1] - tb[2 * b])) % p for b in range(len(tb) // 2)] for tb in tabs]
            total = 0
            for c, which in terms:
                for b in range(len(at[0])):
                    prod = c
                    for i in which:
                        prod = prod * at[i][b] % p
                    total += prod
            ys.append(total % p)
        out.append(interpolate(ys, p))
        tabs = [fold(tb, r[j], p) for tb in tabs]
    return out, [tb[0] for tb in tabs]


def prove_linear(inst, public, private, ch, kzg_tau):
    p = inst["p"]
    s_x, h, s = sizes(inst)
    w, z = tables(inst, public, private)
    tau, rx, r_abc, ry = ch["tau"], ch["rx"], ch["r_abc"], ch["ry"]
    az, bz, cz = products(*row_major(inst), z, p)
    outer, last = rounds_linear([M.eq_basis(tau, p), az, bz, cz], [(1, (0, 1, 2)), (p - 1, (0, 3))], 3, rx, p)
    m_r = bind(*col_major(inst), M.eq_basis(rx, p), r_abc, p)
    inner, _ = rounds_linear([m_r, z], [(1, (0, 1))], 2, ry, p)
    quotients, v_w = M.open_(w, ry[:h], kzg_tau, p)
    return {"commitment": M.commit(w, kzg_tau, p), "outer": outer, "evals": tuple(last[1:]), "inner": inner, "v_w": v_w,
            "opening": quotients}


def satisfied(inst, public, private):
    p = inst["p"]
    _, z = tables(inst, public, private)
    az, bz, cz = products(*row_major(inst), z, p)
    return all(a * b % p == c for a, b, c in zip(az, bz, cz))


def random_instance(rnd, p, n_row, n_col, n_public, per_row=3):
    """(instance, public, private): random A and B rows of up to `per_row` entries (repeats included) and a C row of two entries
    solved for the witness, which is random and non-zero"""
    wit = [1] + [rnd.randrange(1, p) for _ in range(n_col - 1)]
    inst = {"A": [], "B": [], "C": [], "n_row": n_row, "n_col": n_col, "n_public": n_public, "p": p}
    for r in range(n_row):
        sums = []
        for name in "AB":
            row = [(rnd.randrange(n_col), rnd.randrange(p)) for _ in range(rnd.randrange(per_row + 1))]
            inst[name] += [(r, c, v) for c, v in row]
            sums.append(sum(v * wit[c] for c, v in row) % p)
        c0, c1, v0 = rnd.randrange(n_col), rnd.randrange(n_col), rnd.randrange(p)
        v1 = (sums[0] * sums[1] - v0 * wit[c0]) * pow(wit[c1], -1, p) % p
        inst["C"] += [(r, c0, v0), (r, c1, v1)]
    return inst, wit[:n_public], wit[n_public:]


def random_challenges(rnd, inst):
    p = inst["p"]
    s_x, h, s = sizes(inst)
    draw = lambda k: [rnd.randrange(p) for _ in range(k)]  # noqa: E731
    return {"tau": draw(s_x), "rx": draw(s_x), "r_abc": tuple(draw(3)), "ry": draw(s)}, draw(h)


# ---- the verifier -----------------------------------------------------------------------------------------------------------
def public_mle(public, point, p):
    return sum(v * e for v, e in zip(public, M.eq_basis(point, p))) % p


def verify(inst, public, proof, ch, kzg_tau):
    p = inst["p"]
    s_x, h, s = sizes(inst)
    tau, rx, r_abc, ry = ch["tau"], ch["rx"], ch["r_abc"], ch["ry"]
    if len(public) != inst["n_public"] or len(proof["outer"]) != s_x or len(proof["inner"]) != s or len(proof["opening"]) != h:
        return False
    if any(len(c) != 4 for c in proof["outer"]) or any(len(c) != 3 for c in proof["inner"]):
        return False
    claim = 0
    for coeffs, r in zip(proof["outer"], rx):
        if (horner(coeffs, 0, p) + horner(coeffs, 1, p)) % p != claim:
            return False
        claim = horner(coeffs, r, p)
    va, vb, vc = proof["evals"]
    if eq_point(tau, rx, p) * (va * vb - vc) % p != claim:
        return False
    claim = sum(r * v for r, v in zip(r_abc, proof["evals"])) % p
    for coeffs, r in zip(proof["inner"], ry):
        if (horner(coeffs, 0, p) + horner(coeffs, 1, p)) % p != claim:
            return False
        claim = horner(coeffs, r, p)
    v_z = ((1 - ry[h]) * proof["v_w"] + ry[h] * public_mle([v % p for v in public] + [0] * ((1 << h) - len(public)), ry[:h], p)) % p
    m_r = bind(*col_major(inst), M.eq_basis(rx, p), r_abc, p)
    if M.evaluate(m_r, ry, p) * v_z % p != claim:
        return False
    # the pairing check in the exponent: C - v_w == sum_k (tau_k - z_k) Q_k
    rhs = sum((kzg_tau[k] - ry[k]) * q for k, q in enumerate(proof["opening"]))
    return (proof["commitment"] - proof["v_w"] - rhs) % p == 0
