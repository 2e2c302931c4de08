// k_xspec_cu1024 (pp_xspec1024cu.h) in a translation unit -- a code object -- of its own.
//
// In one module with the library's other kernels the compiler selects other instructions for the lane arithmetic of
// k_xspec_q1024<double, false>'s row loop (two VALU fewer, nothing else moves; wherever in the module the new kernel is
// instantiated), and that loop is pinned instruction by instruction (tests/test_row_loop_valu_count.py).  Apart, neither
// kernel knows of the other (profiles/cu_tables_ab.txt has the comparison).  The headers define kernels that are no
// templates, so this unit sees them in a namespace of its own: nothing of it but the two functions below is referenced
// from outside.  The cost: those kernels (26 of them) are compiled a second time and sit in this unit's code object
// unused; with them, the new kernel and its ticket function the library grows from 9.5 to 10.8 MB and the build by
// under a minute.
#include "../../include/pp_toas.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#define pp pp_cu_unit
#include "pp_tail.h"
#include "pp_xspec1024cu.h"
#undef pp

// the size of the kernel's one dynamic LDS block, announced once (it is past the 64 KB a launch may ask for unannounced)
extern "C" __attribute__((visibility("hidden"))) int pp_cu1024_prepare(void) {
    return (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&pp_cu_unit::k_xspec_cu1024<double>),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, pp_cu_unit::CU_LDS_BYTES);
}

// xspec_args: the caller's XspecArgs (the same header, the same layout).  One workgroup of eight waves per CU, at most
// one wave per row (a wave walks chunks of 32 rows: in a small batch most waves pass the barrier and leave, or take
// tickets, as the surplus workgroups of k_xspec_q1024's grid of min(nrows, capacity) do).
extern "C" __attribute__((visibility("hidden"))) void pp_cu1024_launch(const void* xspec_args, long long nrows, int ncu, hipStream_t stream) {
    const pp_cu_unit::XspecArgs& xa = *static_cast<const pp_cu_unit::XspecArgs*>(xspec_args);
    const long long want = (nrows + pp_cu_unit::CU_WAVES - 1) / pp_cu_unit::CU_WAVES;
    const dim3 grid((unsigned)(want < 1 ? 1 : want > ncu ? ncu : want));
    hipLaunchKernelGGL(pp_cu_unit::k_xspec_cu1024<double>, grid, dim3(64 * pp_cu_unit::CU_WAVES), pp_cu_unit::CU_LDS_BYTES,
                       stream, xa);
}
