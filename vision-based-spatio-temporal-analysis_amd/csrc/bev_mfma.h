// bev_mfma.h -- internal: what the MFMA conv / weight-gradient sources (bev_conv*.hip, bev_train.hip, bev_effnet*.hip)
// used to restate each: the XCD block order, the LDS-DMA copy, the range-checked buffer resource, and on the host the
// launch status, the CU count and the conv output size.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// XCD-aware block order.  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs; this maps id `bid`
// of a grid of `nb` so that each XCD walks one contiguous run of the logical order: blocks next to each other there
// (the N tiles that read the same A rows) run on one XCD and share its L2.
__device__ __forceinline__ unsigned xcd_block(unsigned bid, unsigned nb) {
    const unsigned q = nb / 8, r = nb % 8, xc = bid % 8;
    return (xc < r ? xc * (q + 1) : r * (q + 1) + (xc - r) * q) + bid / 8;
}

// LDS address (byte offset in the workgroup's LDS) of a __shared__ object
__device__ __forceinline__ unsigned lds_addr(const void *p) {
    return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// LDS-DMA: every lane copies its 16 bytes at src straight to LDS, lane l to dst + 16 l (global_load_lds_dwordx4: no
// staging VGPRs, no ds_write).  dst is wave-uniform and travels in m0, which is restored.
__device__ __forceinline__ void lds_dma16(const void *src, unsigned dst_any) {
    const unsigned dst = (unsigned)__builtin_amdgcn_readfirstlane((int)dst_any);  // wave-uniform LDS address
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(src), "s"(dst)
        : "memory");
}

// Raw buffer resource over [p, p + bytes): the part of an address that sits in the VGPR offset is range-checked, so
// loads past the end return 0 and stores there are dropped.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void *p, int64_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)(uint32_t)bytes, 0x00020000);
}

// status of the launch just made: 0 or the hipError_t
static inline int last() { return (int)hipGetLastError(); }

// compute units of the current device, asked once per source; 256 where the runtime does not say
static inline int cu_count() {
    static int num_cu = 0;
    if (num_cu == 0) {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
            n = 256;
        num_cu = n;
    }
    return num_cu;
}

// Output rows (columns) of a conv over `in` rows: the expression the entry points check Ho / Wo against
// (bev_native.py _out_hw).  The callers have checked stride > 0.
static inline int conv_out(int in, int pad, int dil, int k, int stride) {
    return (in + 2 * pad - dil * (k - 1) - 1) / stride + 1;
}
