// guard_band.h -- TEST ONLY: device arrays between guard bands, shared by the probes of tests/hip/.
//
// Guarded<T> holds n elements of T between two bands of g elements filled with the byte 0xA5; the n themselves are zeroed, or copied
// from `src`.  get() copies the n elements back and compares both bands: a kernel that wrote outside its array, at a size that is no
// multiple of the workgroup for instance, is found without leaving the allocation.  The first array found touched is noted in
// GuardStatus, whose code() is the HIP error, or PT_GUARD_TOUCHED + the array's number, or 0.
#ifndef PT_TEST_GUARD_BAND_H
#define PT_TEST_GUARD_BAND_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <vector>

constexpr int PT_GUARD_TOUCHED = 100000;
constexpr unsigned char kGuardByte = 0xA5;

struct GuardStatus {
    hipError_t err = hipSuccess;
    int touched = 0; // 1 + the number of the first array whose guard band was written
    int arrays = 0;
    bool ok() const {
        return err == hipSuccess;
    }
    void operator()(hipError_t e) {
        if(err == hipSuccess && e != hipSuccess) {
            err = e;
        }
    }
    int code() const {
        return err != hipSuccess ? static_cast<int>(err) : (touched != 0 ? PT_GUARD_TOUCHED + touched - 1 : 0);
    }
};

template<typename T>
struct Guarded {
    T *base = nullptr;
    size_t n, g;
    int id;
    GuardStatus &st;
    Guarded(GuardStatus &status, size_t count, size_t guard, const T *src = nullptr) : n(count), g(guard), id(status.arrays++), st(status) {
        if(!st.ok()) {
            return;
        }
        st(hipMalloc(reinterpret_cast<void **>(&base), (n + 2 * g) * sizeof(T)));
        if(st.ok()) {
            st(hipMemset(base, kGuardByte, (n + 2 * g) * sizeof(T)));
        }
        if(st.ok() && n > 0) {
            st(src != nullptr ? hipMemcpy(base + g, src, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(base + g, 0, n * sizeof(T)));
        }
    }
    Guarded(const Guarded &) = delete;
    Guarded &operator=(const Guarded &) = delete;
    ~Guarded() {
        if(base != nullptr) {
            (void)hipFree(base);
        }
    }
    T *p() const {
        return base == nullptr ? nullptr : base + g;
    }
    void get(T *dst) {
        if(st.ok() && n > 0) {
            st(hipMemcpy(dst, base + g, n * sizeof(T), hipMemcpyDeviceToHost));
        }
        for(size_t first : {size_t(0), g + n}) {
            if(!st.ok() || g == 0) {
                return;
            }
            std::vector<unsigned char> h(g * sizeof(T));
            st(hipMemcpy(h.data(), base + first, h.size(), hipMemcpyDeviceToHost));
            for(unsigned char b : h) {
                if(st.ok() && b != kGuardByte && st.touched == 0) {
                    st.touched = id + 1;
                }
            }
        }
    }
};

#endif
