// preprocess_choice.h — which form of preprocess_backward_kernel (preprocess_bwd.hip) a backward launches, and the forward's rule for
// staging the SH rows through LDS (preprocess.hip), as host arithmetic on plain values: the named form, the ONE list of base forms that are
// instantiated, the rule, the reason a chained call is refused, the raw name a launch is recorded under.  In the mould of kernel_choice.h: no
// HIP, no switches(), no error reporting — launch_preprocess_backward launches what choose_preprocess_backward says.  Compiles with a plain
// C++17 compiler (das3r_debug_choose_preprocess_backward / das3r_debug_preprocess_backward_name: tests/test_preprocess_choice_host.py drives
// every row of the rule on the CPU, tests/preprocess_choice_host_main.cpp every combination of its inputs).
#pragma once

namespace das3r {

// A form = the nine template arguments of preprocess_backward_kernel, in their order (the mangled names and the raw names of the launch
// records depend on it).  What each one means is written at the kernel.
struct PreprocessForm {
    bool has_sh, has_cov, stage_in, stage_out, deg0, chain, depth, jac, aa;
};

// The base forms that are instantiated, each times DEPTH times AA (17 x 4 = 68 kernels):
//   X(HAS_SH, HAS_COV, STAGE_IN, STAGE_OUT, DEG0, CHAIN, JAC)
// The ORDER is the order the kernels are instantiated in and with it the order of the code objects in the library: it stays
// (docs/ledger.md (ci): a moved launch reordered the instantiations and changed the fatbin).
#define DAS3R_PREPROCESS_BACKWARD_FORMS(X)                                                                     \
    X(true, false, false, false, true, true, false)    /* chained, degree 0 */                                 \
    X(true, false, false, false, false, true, true)    /* chained, the forward's Jacobian planes */            \
    X(true, false, false, false, false, true, false)   /* chained, SH rows */                                  \
    X(true, true, false, true, false, false, true)     /* Jacobian planes, cov3D, dL_dsh rows through LDS */   \
    X(true, true, false, false, false, false, true)                                                            \
    X(true, false, false, true, false, false, true)                                                            \
    X(true, false, false, false, false, false, true)                                                           \
    X(true, false, true, true, false, false, false)    /* SH rows in and dL_dsh rows out through LDS */        \
    X(true, false, false, true, false, false, false)                                                           \
    X(true, false, false, false, true, false, false)                                                           \
    X(true, false, false, false, false, false, false)                                                          \
    X(true, true, true, true, false, false, false)     /* the same four with cov3D */                          \
    X(true, true, false, true, false, false, false)                                                            \
    X(true, true, false, false, true, false, false)                                                            \
    X(true, true, false, false, false, false, false)                                                           \
    X(false, false, false, false, false, false, false) /* precomputed colours */                               \
    X(false, true, false, false, false, false, false)

static inline bool same_base_form(const PreprocessForm &f, bool has_sh, bool has_cov, bool stage_in, bool stage_out, bool deg0, bool chain, bool jac) {
    return f.has_sh == has_sh && f.has_cov == has_cov && f.stage_in == stage_in && f.stage_out == stage_out && f.deg0 == deg0 && f.chain == chain &&
           f.jac == jac;
}
// position of the form's base form in the list, -1: not instantiated
static inline int preprocess_backward_base_index(const PreprocessForm &f) {
    int k = 0;
#define X(SH, COV, SI, SO, D0, CH, J)                          \
    if (same_base_form(f, SH, COV, SI, SO, D0, CH, J)) return k; \
    k++;
    DAS3R_PREPROCESS_BACKWARD_FORMS(X)
#undef X
    return -1;
}
// The raw name a launch of the form is recorded under (das3r_profile_report): the text of the instantiation as a launch site spells it,
// parentheses included.  Null: the form is not instantiated.  For the tests: the launch site does not ask this function, DAS3R_LAUNCH
// stringifies the instantiation it launches, and tests/test_gpu_preprocess_forms.py holds the one against the other.
static inline const char *preprocess_backward_name(const PreprocessForm &f) {
#define X(SH, COV, SI, SO, D0, CH, J)                                                                                                      \
    if (same_base_form(f, SH, COV, SI, SO, D0, CH, J)) {                                                                                   \
        if (f.aa) return f.depth ? "(preprocess_backward_kernel<" #SH ", " #COV ", " #SI ", " #SO ", " #D0 ", " #CH ", true, " #J ", true>)"  \
                                 : "(preprocess_backward_kernel<" #SH ", " #COV ", " #SI ", " #SO ", " #D0 ", " #CH ", false, " #J ", true>)"; \
        return f.depth ? "(preprocess_backward_kernel<" #SH ", " #COV ", " #SI ", " #SO ", " #D0 ", " #CH ", true, " #J ", false>)"          \
                       : "(preprocess_backward_kernel<" #SH ", " #COV ", " #SI ", " #SO ", " #D0 ", " #CH ", false, " #J ", false>)";        \
    }
    DAS3R_PREPROCESS_BACKWARD_FORMS(X)
#undef X
    return nullptr;
}

// waves per SIMD the unchained JAC forms are built for: the staged one's 26 KB of LDS would leave room for six workgroups per CU, its
// registers for five (87 VGPRs; at six it spills)
constexpr int JAC_WAVES = 5;
// The AA forms that cannot hold their target without spilling take their own: DEG0 5 waves instead of 6, the unchained JAC forms 4 instead
// of 5, and the chained form with SH rows 2 (its non-AA form, which the same bound of 3 would leave as it is, spills already).
constexpr int pb_waves(const bool DEG0, const bool CHAIN, const bool JAC, const bool AA) {
    return DEG0 ? (CHAIN ? 4 : (AA ? 5 : 6)) : JAC && !CHAIN ? (AA ? JAC_WAVES - 1 : JAC_WAVES) : (AA && CHAIN && !JAC ? 2 : 3);
}

// The FORWARD's rule: the workgroup's SH rows come in through LDS (preprocess_kernel<.., STAGE>, sh_colour_kernel<STAGE>) when a row is
// twelve whole float4 (M == 16, 16-byte aligned) and the active degree reads most of it.  The backward stages its SH input rows by the
// same rule (choose_preprocess_backward: stage_in).
static inline bool sh_rows_staged(bool has_sh, int M, int sh_degree, bool shs_aligned16, bool no_sh_stage) {
    return has_sh && M == 16 && sh_degree >= 2 && shs_aligned16 && !no_sh_stage;
}

struct PreprocessBackwardInputs {
    bool has_sh, has_cov;                      // in->shs / in->cov3D_precomp given
    int M, sh_degree;
    bool shs_aligned16, dL_dshs_aligned16;     // 16-byte alignment of in->shs and of grads->dL_dshs
    bool no_sh_stage;                          // Switches::no_sh_stage
    bool jac_saved;                            // the forward left the Jacobian planes (Layout::g_shjac != 0: flags bit 2, degree >= 2)
    bool chained;                              // das3r_raster_grads.chain
    bool quad_rows;                            // the compositing backward left a row per (instance, quadrant)
    bool depth, aa;                            // dz given (das3r_raster_backward_depth); das3r_raster_saved.flags bit 4
};

// dL_dsh rows leave through LDS (M == 16: 256 rows of twelve whole float4), and with them the per-instance rows come in through it
static inline bool dsh_rows_staged(const PreprocessBackwardInputs &in) {
    return in.has_sh && in.M == 16 && in.dL_dshs_aligned16 && !in.no_sh_stage;
}

// Why a chained call (das3r_raster_grads.chain) is refused, as far as plain values say; the pointers of the chain and of in->pre are
// launch_preprocess_backward's to look at.  The chained forms keep their gradient rows in registers to the end: unstaged SH layouts only.
enum ChainRefusal : int {
    CHAIN_OK = 0,
    CHAIN_NEEDS_SH = 1,         // precomputed colours
    CHAIN_HAS_COV = 2,          // cov3D given: no scales + rotations to chain through
    CHAIN_STAGED_LAYOUT = 3,    // dsh_rows_staged: M == 16 rows through LDS
    CHAIN_QUAD_ROWS = 4,        // quadrant rows (experiments build)
};
static inline ChainRefusal chain_refusal(const PreprocessBackwardInputs &in) {
    if (!in.chained) return CHAIN_OK;
    if (!in.has_sh) return CHAIN_NEEDS_SH;
    if (in.has_cov) return CHAIN_HAS_COV;
    if (dsh_rows_staged(in)) return CHAIN_STAGED_LAYOUT;
    if (in.quad_rows) return CHAIN_QUAD_ROWS;
    return CHAIN_OK;
}

// The form a backward launches (for a chained call: unless chain_refusal says it is refused).  Always one of the instantiated ones
// (tests/preprocess_choice_host_main.cpp walks every combination).
static inline PreprocessForm choose_preprocess_backward(const PreprocessBackwardInputs &in) {
    const bool stage_out = dsh_rows_staged(in);
    const bool jac = in.has_sh && in.jac_saved;
    // (JAC replaces the SH input row: nothing to stage in)
    const bool stage_in = stage_out && sh_rows_staged(in.has_sh, in.M, in.sh_degree, in.shs_aligned16, in.no_sh_stage) && !jac;
    const bool deg0 = in.sh_degree == 0 && !stage_out;   // (the staged forms have no degree-0 variant)
    PreprocessForm f = {in.has_sh, in.has_cov, false, false, false, false, in.depth, false, in.aa};
    if (in.chained) {   // SH rows in an unstaged layout, scales + rotations: whatever else the inputs say
        f.has_sh = true;
        f.has_cov = false;
        f.chain = true;
        f.deg0 = deg0;
        f.jac = !deg0 && jac;
    } else if (jac) {
        f.jac = true;
        f.stage_out = stage_out;
    } else if (in.has_sh) {
        f.stage_in = stage_in;
        f.stage_out = stage_out;
        f.deg0 = deg0;
    }
    return f;
}

}  // namespace das3r
