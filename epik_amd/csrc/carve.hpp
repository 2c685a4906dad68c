// carve.hpp -- one allocation handed out in consecutive parts: what every *_space() of the cohort analyses is a list of.
// Plain C++ (no HIP): epik_amd/host/host_test.cpp has its unit cases.
#ifndef EPIK_AMD_CARVE_HPP
#define EPIK_AMD_CARVE_HPP

#include <cstddef>

namespace epik_amd {

// Every part starts on a multiple of 16 bytes from the base and takes its size rounded up to one; a part of 0 elements takes
// nothing.  With a null base take() gives null pointers and bytes() still the total: the same list sizes the allocation and
// then names its parts, so their order and their sizes are written once.
class Carver {
public:
    explicit Carver(void *base) : base_(static_cast<char *>(base)) {}
    static constexpr size_t rounded(size_t bytes) { return (bytes + 15) / 16 * 16; }
    template <class T>
    T *take(size_t count)
    {
        T *part = base_ ? reinterpret_cast<T *>(base_ + at_) : nullptr;
        at_ += rounded(count * sizeof(T));
        return part;
    }
    size_t bytes() const { return at_; }

private:
    char *base_;
    size_t at_ = 0;
};

}  // namespace epik_amd
#endif
