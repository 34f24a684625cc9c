// One KERNEL SET: yf_kernels.hip.h compiled under the requantisation switch the includer has defined (none, YF_RQ3_DENSE or YF_RQ_FP32) into namespaces
// that end in YF_SET (empty, u or x):
//   yf<set>     56x56: the fused kernel
//   yf160<set>  160x160 (BASELINE configs[4]): the same stage code on band-local buffers (three banded kernels; YF_LAB: also layer by layer over an HBM arena)
// Under YF_DUMP_PROD_ORDER (laboratory) it is ONE namespace instead, yfpd<set>: the 56x56 kernel as a dump build that keeps the PRODUCTION stage order
// (yf_fused56.hip.h, YF_PDUMP) -- per-stage parity of what ships.
// No include guard: yf_engine.hip includes it once per set.  YF_SET and the switch are used up (undefined at the end); YF_DUMP_PROD_ORDER is the includer's.
#define YF_PASTE_(a, b) a##b
#define YF_PASTE(a, b) YF_PASTE_(a, b)
#ifndef YF_DUMP_PROD_ORDER
#define YF_NS YF_PASTE(yf, YF_SET)
#include "yf_kernels.hip.h"
#undef YF_NS
#undef YF_H0
#define YF_NS YF_PASTE(yf160, YF_SET)
#define YF_H0 160
#define YF_GENERIC 1
#include "yf_kernels.hip.h"
#undef YF_GENERIC
#else
#define YF_NS YF_PASTE(yfpd, YF_SET)
#include "yf_kernels.hip.h"
#endif
#undef YF_NS
#undef YF_H0
#undef YF_SET
#undef YF_RQ3_DENSE
#undef YF_RQ_FP32
