// mmv_fused_iq4nl.hip -- the k_mmv_stream instances of one weight format (mmv_fused_impl.h),
// compiled as a translation unit of their own so that the formats build in parallel
#include "mmv_fused_impl.h"

template <> void mi_mmv_launch<MI_TYPE_IQ4_NL>(const mi_mmv_group & g, int variant, hipStream_t s) {
    launch_stream_ord<FmtIQ4NL>(g, variant, s);
}
