// host_tail_check.cpp -- runs msm_host_tail (csrc/msm_host_tail.h), the last stage of every MSM, on (S, T) blocks that are known
// multiples of the generator.  tests/test_host_lib.py chooses the scalars, computes the expected multiple with integers from the
// formula in the tail's comment and compares the affine coordinates printed here.  Cases come on stdin, one after the other:
//   <group> <c> <shape_c> <wide> <groups> <q_first> <pre> <n>     then n scalars (hex, below 2^256), the blocks of h_final in order
//   group: 0 BN254 G1, 1 BN254 G2, 2 BLS12-381 G1, 3 BLS12-381 G2; the reduction shape is that of (shape_c, wide), n = 2 groups (bpr + bpc)
// and one line goes out per case: the base-field components of x then y as hex integers, or "refused: <message>".
// Stand-alone host program, no HIP:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined host_tail_check.cpp && ./a.out < cases
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zksnake_amd/csrc/msm_host_tail.h"
#include "../../zksnake_amd/csrc/curve_consts.h"

using namespace zkmi;

template <class G> static const uint32_t* generator();
template <> const uint32_t* generator<Bn254G1>() { return Bn254Consts::G1_GEN; }
template <> const uint32_t* generator<Bn254G2>() { return Bn254Consts::G2_GEN; }
template <> const uint32_t* generator<Bls381G1>() { return Bls381Consts::G1_GEN; }
template <> const uint32_t* generator<Bls381G2>() { return Bls381Consts::G2_GEN; }

// k G as an XYZZ row in device form (packed words of the 29-bit-limb Montgomery values), zeros for infinity
template <class G>
static void put_multiple(uint32_t* row, const uint32_t k[8]) {
    typedef typename G::F F;
    const uint32_t* g = generator<G>();
    const Affine<F> gen = {F::from_canonical(g), F::from_canonical(g + F::LIMBS)};
    const XYZZ<F> p = xyzz_scalar_mul<F>(gen, k, 8);
    F::store(row, p.X);
    F::store(row + F::LIMBS, p.Y);
    F::store(row + 2 * F::LIMBS, p.ZZ);
    F::store(row + 3 * F::LIMBS, p.ZZZ);
}

static bool read_scalar(uint32_t k[8]) {
    char buf[80];
    if (scanf("%79s", buf) != 1) return false;
    const size_t len = strlen(buf);
    if (len == 0 || len > 64) return false;
    memset(k, 0, 32);
    for (size_t i = 0; i < len; ++i) {
        const char ch = buf[len - 1 - i];
        const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
        if (d < 0) return false;
        k[i / 8] |= (uint32_t)d << (4 * (i % 8));
    }
    return true;
}

template <class G>
static int run_case(int c, const ReduceShape& shape, int groups, int q_first, int pre, int n) {
    constexpr int XW = 4 * G::F::LIMBS, W = G::F::Params::W;
    std::vector<uint32_t> h_final((size_t)n * XW);
    for (int i = 0; i < n; ++i) {
        uint32_t k[8];
        if (!read_scalar(k)) return 2;
        put_multiple<G>(h_final.data() + (size_t)i * XW, k);
    }
    uint64_t out[G::F::LIMBS];   // 2 LIMBS words of 32 bits
    if (msm_host_tail<G>(h_final.data(), (uint32_t)groups, shape, c, q_first, pre != 0, out)) {
        printf("refused: %s\n", last_error_ref().c_str());
        return 0;
    }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(out);
    for (int e = 0; e < 2 * G::F::LIMBS / W; ++e) {
        printf(e ? " " : "");
        for (int i = W - 1; i >= 0; --i) printf("%08x", w[e * W + i]);
    }
    printf("\n");
    return 0;
}

int main() {
    int group, c, shape_c, wide, groups, q_first, pre, n;
    while (scanf("%d %d %d %d %d %d %d %d", &group, &c, &shape_c, &wide, &groups, &q_first, &pre, &n) == 8) {
        ReduceShape shape;
        if (group < 0 || group > 3 || c < 2 || c > 20 || shape_c < 2 || shape_c > 20 || !reduce_shape(shape_c, wide != 0, &shape) || groups < 0 || groups > 16 ||
            q_first < 0 || q_first > 16 || n != 2 * groups * (int)shape.blocks()) {
            fprintf(stderr, "host_tail_check: bad case\n");
            return 2;
        }
        int rc;
        switch (group) {
        case 0: rc = run_case<Bn254G1>(c, shape, groups, q_first, pre, n); break;
        case 1: rc = run_case<Bn254G2>(c, shape, groups, q_first, pre, n); break;
        case 2: rc = run_case<Bls381G1>(c, shape, groups, q_first, pre, n); break;
        default: rc = run_case<Bls381G2>(c, shape, groups, q_first, pre, n); break;
        }
        if (rc) {
            fprintf(stderr, "host_tail_check: bad scalar\n");
            return rc;
        }
    }
    return 0;
}
