// The device memory of a handle: every hipMalloc of a handle goes through the ibh_owner member of its struct, whose
// destructor frees it all -- with the handle, or with the std::unique_ptr that holds a handle while its create function can
// still fail.  The pointer fields of the handles stay bare pointers (they are copied into kernel arguments); the owner only
// remembers what to free.  Host only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

int ibh_fail(int code, const char* what, const char* file, int line);

// what the owners of all live handles hold (ibh_owned_device_memory); not part of the ABI
__attribute__((visibility("hidden"))) inline std::atomic<int64_t> ibh_owned_bytes{0}, ibh_owned_buffers{0};

struct ibh_owner {
    std::vector<void*> bufs;
    int64_t bytes = 0;

    ibh_owner() = default;
    ibh_owner(const ibh_owner&) = delete;
    ibh_owner& operator=(const ibh_owner&) = delete;
    ~ibh_owner() {
        for (void* b : bufs) hipFree(b);
        ibh_owned_bytes -= bytes;
        ibh_owned_buffers -= (int64_t)bufs.size();
    }

    // *dptr = n uninitialised elements, or null for n = 0
    template <class T>
    int alloc(T** dptr, size_t n) {
        *dptr = nullptr;
        if (n == 0) return 0;
        void* b = nullptr;
        const hipError_t e = hipMalloc(&b, n * sizeof(T));
        if (e != hipSuccess) return ibh_fail((int)e, hipGetErrorString(e), __FILE__, __LINE__);
        bufs.push_back(b);
        bytes += (int64_t)(n * sizeof(T));
        ibh_owned_bytes += (int64_t)(n * sizeof(T));
        ibh_owned_buffers += 1;
        *dptr = (T*)b;
        return 0;
    }
    // *dptr = a copy of host[0 .. n), or null for n = 0
    template <class T>
    int upload(T** dptr, const T* host, size_t n) {
        if (const int rc = alloc(dptr, n)) return rc;
        if (n == 0) return 0;
        const hipError_t e = hipMemcpy(*dptr, host, n * sizeof(T), hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : ibh_fail((int)e, hipGetErrorString(e), __FILE__, __LINE__);
    }
    template <class T>
    int upload(T** dptr, const std::vector<T>& host) {
        return upload(dptr, host.data(), host.size());
    }
};
