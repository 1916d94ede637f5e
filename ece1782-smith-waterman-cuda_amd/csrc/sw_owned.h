// sw_owned.h — the one owner of a handle-like value (a pointer, an event, a
// stream): move-only, released exactly once through Release, which is never
// called on the empty value T{}.  No HIP here: sw_host.h names the four
// owners the host driver uses, tests/native/owned_check.cpp counts releases.
#pragma once

#include <utility>

namespace swk {

template <class T, void (*Release)(T)>
class Owned {
public:
    Owned() = default;
    explicit Owned(T v) : v_(v) {}
    Owned(Owned&& o) noexcept : v_(o.release()) {}
    Owned& operator=(Owned&& o) noexcept {  // releases what it held first
        if (this != &o) {
            reset();
            v_ = o.release();
        }
        return *this;
    }
    ~Owned() { reset(); }  // (no copy: the move members delete it)

    T get() const { return v_; }
    void reset() {  // release now
        if (v_ != T{}) Release(release());
    }
    T release() { return std::exchange(v_, T{}); }  // give up ownership

private:
    T v_{};
};

}  // namespace swk
