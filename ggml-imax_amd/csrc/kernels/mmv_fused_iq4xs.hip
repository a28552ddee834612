// mmv_fused_iq4xs.hip -- the k_mmv_stream instances of one weight format (mmv_fused_impl.h),
// compiled as a translation unit of their own so that the formats build in parallel
#include "mmv_fused_impl.h"

template <> void mi_mmv_launch<MI_TYPE_IQ4_XS>(const mi_mmv_group & g, int variant, hipStream_t s) {
    launch_stream_ord<FmtIQ4XS>(g, variant, s);
}
