// Host side of the streamed pair kernel (qs_pair4s.h): eligibility and dispatch of the complex128 fused passes (pair4c_try)
// and of the first pass of a real tensor against complex coefficients (pair4m_try).
#include "qs_pair4s.h"

namespace qs {

namespace {

int launch_any(int n4, bool real_in, const Pair4Args& g, hipStream_t stream) {
    int rc = 1;
    if (real_in) {
        rc = launch_pair4m_a(n4, g, stream);
        if (rc == 1) rc = launch_pair4m_b(n4, g, stream);
        return rc;
    }
    rc = launch_pair4s_a(n4, g, stream);
    if (rc == 1) rc = launch_pair4s_b(n4, g, stream);
    if (rc == 1) rc = launch_pair4s_c(n4, g, stream);
    if (rc == 1) rc = launch_pair4s_d(n4, g, stream);
    return rc;
}

}  // namespace

// Out_t = Lm . In_t . R for t < nitems, complex128 (element strides); QS_OK / error after launching, 1 = not eligible.
int pair4c_try(int dtype, const FusedPass& pass, int tensor_is_b, hipStream_t stream) {
    const int64_t L = pass.L, M = pass.M, nitems = pass.nitems;
    if (dtype != QS_C128) return 1;
    if (L < 5 || M < 5 || L > 64 || M > 64) return 1;       // (up to 4 orbitals: qs_small4.hip)
    const int n4 = (int)cdiv(L, 4);
    if (n4 != (int)cdiv(M, 4)) return 1;
    if (pass.in_col != 1 && pass.in_item != 1) return 1;
    if (!aligned(pass.in, 16) || !aligned(pass.out, 16) || !aligned(pass.R, 16) || !aligned(pass.Lm, 16)) return 1;
    if (nitems < 1 || nitems >= (int64_t(1) << 31)) return 1;
    Pair4Args g = fused_args<Pair4Args>(pass, 2);
    g.tensor_is_b = tensor_is_b;
    return launch_any(n4, false, g, stream);
}

// The same for REAL items against complex R and Lm (element strides of `in` count doubles, those of `out` complex
// elements): the first pass of a real tensor against complex coefficients.  Slabs only (in_col == 1).
int pair4m_try(const FusedPass& pass, hipStream_t stream) {
    const int64_t L = pass.L, M = pass.M, nitems = pass.nitems;
    if (L < 5 || M < 5 || L > 56 || M > 56) return 1;
    const int n4 = (int)cdiv(L, 4);
    if (n4 != (int)cdiv(M, 4)) return 1;
    if (pass.in_col != 1) return 1;
    if (!aligned(pass.in, 8) || !aligned(pass.out, 16) || !aligned(pass.R, 16) || !aligned(pass.Lm, 16)) return 1;
    if (nitems < 1 || nitems >= (int64_t(1) << 31)) return 1;
    return launch_any(n4, true, fused_args<Pair4Args>(pass, 2), stream);
}

}  // namespace qs
