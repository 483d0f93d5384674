// Launch of the imaginary-time fold kernel (sse_itime.hip.h): group observables and bond counts of every replica.
#include "sse_itime.hip.h"
namespace sse {
hipError_t launch_itime(hipStream_t stream, const DevBatch &B, const ItimeArgs &A) {
    const size_t lds = 4 * itime_carve(A.W, B.N, B.nwords, B.Nb, A.G.ngroups, A.nv, A.hist_lds != 0u, A.csr_lds != 0u).words;
    return launch_lds(A.csr_lds ? itime_kernel<true> : itime_kernel<false>, dim3(B.R), dim3(A.W * 64u), lds, stream, B, A);
}
} // namespace sse
