// launch_record_runtime.cpp -- a recording stand-in for the part of the HIP runtime that a kernel unit's host code calls
// (tools/launch_record.py links it where the runtime would be): kernel registration, the <<< >>> call configuration, hipLaunchKernel and
// hipGetLastError.  Nothing is launched and no device is opened; every launch is written down for launch_record_driver.hip to print.
#include <hip/hip_runtime_api.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace {

// host handle -> kernel name, filled by the objects' static constructors (plain arrays: they need no constructor of their own)
constexpr int kMaxKernels = 16384;
const void* g_handle[kMaxKernels];
const char* g_name[kMaxKernels];
int g_kernels;

struct {
    dim3 grid, block;
    size_t shmem;
    hipStream_t stream;
} g_config;

size_t g_arg_bytes;
int g_launches;
char g_line[1024];
hipError_t g_last_error;

uint64_t fnv1a(const void* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; i++) h = (h ^ static_cast<const uint8_t*>(p)[i]) * 0x100000001b3ull;
    return h;
}

}  // namespace

extern "C" {

// ---- what the driver calls around every launcher ---------------------------------------------------------------------------------
// the next launch hands arg_bytes bytes to its kernel; an error of some earlier call is left behind, as a host framework may leave one
void launch_record_begin(size_t arg_bytes) {
    g_arg_bytes = arg_bytes, g_launches = 0, g_line[0] = 0;
    g_last_error = hipErrorUnknown;
}
// launches since launch_record_begin, and the last one's line
int launch_record_end(const char** line) {
    *line = g_line;
    return g_launches;
}

// ---- what hipcc's host code calls -------------------------------------------------------------------------------------------------
void** __hipRegisterFatBinary(const void*) {
    static void* module;
    return &module;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* handle, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
    if (g_kernels < kMaxKernels) g_handle[g_kernels] = handle, g_name[g_kernels] = device_name, g_kernels++;
}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shmem, hipStream_t stream) {
    g_config = {grid, block, shmem, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shmem, hipStream_t* stream) {
    *grid = g_config.grid, *block = g_config.block, *shmem = g_config.shmem, *stream = g_config.stream;
    return hipSuccess;
}

hipError_t hipLaunchKernel(const void* handle, dim3 grid, dim3 block, void** args, size_t shmem, hipStream_t stream) {
    const char* name = "?";
    for (int i = 0; i < g_kernels; i++)
        if (g_handle[i] == handle) name = g_name[i];
    g_launches++;
    snprintf(g_line, sizeof(g_line), "%s grid=%u,%u,%u block=%u,%u,%u shmem=%zu stream=%p args=%zu:%016llx", name, grid.x, grid.y, grid.z, block.x, block.y,
             block.z, shmem, (void*)stream, g_arg_bytes, (unsigned long long)fnv1a(args[0], g_arg_bytes));
    g_last_error = hipSuccess;
    return hipSuccess;
}

hipError_t hipGetLastError() {
    const hipError_t e = g_last_error;
    g_last_error = hipSuccess;
    return e;
}

hipError_t hipGetDevice(int* device) {
    *device = 0;
    return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t, int) {
    *value = 256;
    return hipSuccess;
}

}  // extern "C"
