// Host-side glue of the C-ABI translation units (engine.hip, ops_abi.hip, vit.hip, collective.hip): the error setters,
// the argument checks and the storage-type dispatch every `mdd_*` entry point is written with.  Nothing here runs on
// the device.
#pragma once
#include <type_traits>
#include <vector>

#include "common.h"
#include "mdd_hip.h"

// the text mdd_last_error() returns (engine.hip owns it); the value is what the entry point returns
int mdd_set_error(hipError_t e, const char* what);
int mdd_set_error_msg(int code, const char* msg);

#define CHECK_ARG(cond, msg) \
  do { if (!(cond)) return mdd_set_error_msg(2, "mdd: invalid argument: " msg); } while (0)
#define CHECK_STORAGE(dtype) \
  CHECK_ARG((dtype) == MDD_DTYPE_F32 || (dtype) == MDD_DTYPE_BF16, "dtype must be MDD_DTYPE_F32 or MDD_DTYPE_BF16")
#define POST_LAUNCH(what) HIP_CHECK_RET(hipGetLastError())

// the type a tag pointer of the dispatchers below names: `using AT = tag_t<decltype(tag)>;`
template <class P> using tag_t = std::remove_pointer_t<P>;

// f(tag) with a null float* / bf16* naming the storage type of `dtype` (MDD_DTYPE_BF16X2 and MDD_DTYPE_F32_BF16OPS
// store fp32)
template <class F> void with_storage(int dtype, F&& f) {
  if (dtype == MDD_DTYPE_BF16) f((bf16*)nullptr); else f((float*)nullptr);
}
// f(scalar tag, storage tag): the scalar is Dual for a tangent call, float for a primal one.  A primal kernel ignores
// its tangent pointers (ldS / stS, common.h), so both forms take the same argument list
template <class F> void with_scalar_storage(bool tangent, int dtype, F&& f) {
  with_storage(dtype, [&](auto* at) {
    if (tangent) f((Dual*)nullptr, at); else f((float*)nullptr, at);
  });
}
// ConvGeom::prec of an op-level dtype
inline int op_prec(int dtype) { return dtype == MDD_DTYPE_BF16X2 ? 1 : (dtype == MDD_DTYPE_F32_BF16OPS ? 2 : 0); }

// descriptors to the device, launch(device pointer) on st, and the stream drained before they are freed again
template <class D, class F> int with_device_descs(const std::vector<D>& descs, hipStream_t st, F&& launch) {
  D* dev = nullptr;
  HIP_CHECK_RET(hipMalloc((void**)&dev, descs.size() * sizeof(D)));
  hipError_t e = hipMemcpy(dev, descs.data(), descs.size() * sizeof(D), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    launch(dev);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  (void)hipFree(dev);
  HIP_CHECK_RET(e);
  return 0;
}
