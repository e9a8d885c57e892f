// Which form of preprocess_backward_kernel a backward launches (das3r_amd/csrc/preprocess_choice.h), over EVERY combination of the rule's
// inputs: the chosen form is one of the instantiated ones, it violates none of the kernel's static_asserts, the chained forms are what
// the kernel's chain needs, and the forward's staging rule agrees with stage_in's definition.  Includes only preprocess_choice.h; built with
// -fsanitize=address,undefined and run by tests/test_preprocess_choice_host.py.  Exits non-zero on a wrong answer.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "../das3r_amd/csrc/preprocess_choice.h"

using namespace das3r;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "preprocess_choice_host: %s failed (line %d, combination %ld)\n", #c, __LINE__, combos); return 1; } } while (0)

int main() {
    long combos = 0;
    // the list itself: 17 distinct base forms, each obeying the kernel's static_asserts; 68 distinct names
    int listed = 0;
    std::set<std::string> names;
    const bool yn[2] = {false, true};
#define X(SH, COV, SI, SO, D0, CH, J)                                                            \
    {                                                                                            \
        const PreprocessForm f = {SH, COV, SI, SO, D0, CH, false, J, false};                     \
        CHECK(preprocess_backward_base_index(f) == listed);                                      \
        CHECK(!(J && (SI || D0)));                                                               \
        CHECK(!CH || (!SO && SH && !COV));                                                       \
        CHECK(!SI || SO);                                                                        \
        for (bool depth : yn)                                                                    \
            for (bool aa : yn) {                                                                 \
                PreprocessForm g = f;                                                            \
                g.depth = depth;                                                                 \
                g.aa = aa;                                                                       \
                const char *n = preprocess_backward_name(g);                                     \
                CHECK(n != nullptr && strncmp(n, "(preprocess_backward_kernel<", 28) == 0);     \
                names.insert(n);                                                                 \
            }                                                                                    \
        listed++;                                                                                \
    }
    DAS3R_PREPROCESS_BACKWARD_FORMS(X)
#undef X
    CHECK(listed == 17);
    CHECK(names.size() == 68);
    const PreprocessForm unlisted = {false, false, true, true, false, false, false, false, false};   // staged SH rows without SH rows
    CHECK(preprocess_backward_base_index(unlisted) == -1 && preprocess_backward_name(unlisted) == nullptr);

    // every combination of the inputs
    const int Ms[] = {0, 1, 4, 9, 15, 16, 17, 25};
    const int degrees[] = {0, 1, 2, 3};
    std::set<int> reached;
    for (int bits = 0; bits < (1 << 10); bits++)
        for (int M : Ms)
            for (int deg : degrees) {
                combos++;
                PreprocessBackwardInputs in;
                in.has_sh = bits & 1;
                in.has_cov = bits & 2;
                in.shs_aligned16 = bits & 4;
                in.dL_dshs_aligned16 = bits & 8;
                in.no_sh_stage = bits & 16;
                in.jac_saved = bits & 32;
                in.chained = bits & 64;
                in.quad_rows = bits & 128;
                in.depth = bits & 256;
                in.aa = bits & 512;
                in.M = M;
                in.sh_degree = deg;
                const ChainRefusal why = chain_refusal(in);
                const PreprocessForm f = choose_preprocess_backward(in);
                // the reasons, in the order they are looked at
                const bool stage_out = in.has_sh && M == 16 && in.dL_dshs_aligned16 && !in.no_sh_stage;
                CHECK(dsh_rows_staged(in) == stage_out);
                if (!in.chained) CHECK(why == CHAIN_OK);
                else if (!in.has_sh) CHECK(why == CHAIN_NEEDS_SH);
                else if (in.has_cov) CHECK(why == CHAIN_HAS_COV);
                else if (stage_out) CHECK(why == CHAIN_STAGED_LAYOUT);
                else if (in.quad_rows) CHECK(why == CHAIN_QUAD_ROWS);
                else CHECK(why == CHAIN_OK);
                // instantiated, and within the kernel's static_asserts
                const int base = preprocess_backward_base_index(f);
                CHECK(base >= 0 && base < listed);
                CHECK(preprocess_backward_name(f) != nullptr);
                CHECK(!(f.jac && (f.stage_in || f.deg0)));
                CHECK(!f.chain || (!f.stage_out && f.has_sh && !f.has_cov));
                CHECK(f.depth == in.depth && f.aa == in.aa && f.chain == in.chained);
                if (why == CHAIN_OK) {   // a call that is launched: the form is the inputs' own
                    reached.insert(base);
                    CHECK(f.has_sh == in.has_sh && f.has_cov == in.has_cov);
                    CHECK(f.stage_out == stage_out);
                    CHECK(f.jac == (in.has_sh && in.jac_saved && !(in.chained && deg == 0)));
                    // the forward's rule and stage_in: SH input rows are staged when the forward staged them, the dL_dsh rows leave
                    // through LDS too, and the Jacobian planes do not replace the row
                    const bool fwd = sh_rows_staged(in.has_sh, M, deg, in.shs_aligned16, in.no_sh_stage);
                    CHECK(fwd == (in.has_sh && M == 16 && deg >= 2 && in.shs_aligned16 && !in.no_sh_stage));
                    CHECK(f.stage_in == (fwd && stage_out && !f.jac));
                    CHECK(f.deg0 == (in.has_sh && deg == 0 && !stage_out && !(f.jac && !f.chain)));
                }
            }
    CHECK(reached.size() == 17);   // no base form is instantiated for nothing
    printf("all checks passed (%ld combinations, %d base forms)\n", combos, listed);
    return 0;
}
