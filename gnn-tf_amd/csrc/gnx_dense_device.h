// What the two matrix-core units share (gnx_dense.hip: the forward product; gnx_dense_wgrad.hip: its weight gradient): the MFMA
// operand type, the preamble of a persistent launch and the switch of a tuning build.  Internal linkage, as in gnx_spmm_device.h.
#pragma once
#include "gnx_spmm_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// the CU count of device `dev`, asked of the runtime once per device (256 where the query fails or there is no current device)
inline int device_cus(int dev) {
    static std::atomic<int> known[64] = {};
    const bool slot = dev >= 0 && dev < 64;
    int cus = slot ? known[dev].load(std::memory_order_relaxed) : 0;
    if (cus > 0) return cus;
    cus = 256;
    if (dev >= 0) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (slot) known[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

// Before the launch of a persistent kernel (k_dense_ring, k_dense_wreg, k_wgrad_acc: the CU's LDS as dynamic shared memory, a grid
// sized by the CUs): raises the kernel's dynamic-LDS limit to 160 KB, once per device and kernel instantiation.  Returns the CU count
// of the current device, or a negative GNX_ERR_*.
template <auto Kernel>
int persistent_launch() {
    static PerDeviceOnce configured;
    const int dev = PerDeviceOnce::device();
    if (configured.need(dev)) {
        GNX_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10));
        configured.set(dev);
    }
    return device_cus(dev);
}

// tuning_switch("GNX_X"): is the kernel family in use?  Tuning builds read the variable once (per place of use: every name has one),
// and a value beginning with 0 turns the family off, for A/B runs; the product build compiles no getenv, only the constant.
#ifdef GNX_TUNING
#define tuning_switch(NAME) ([] { static const bool on = [] { const char *e = getenv(NAME); return !(e && e[0] == '0'); }(); return on; }())
#else
#define tuning_switch(NAME) true
#endif

}  // namespace
