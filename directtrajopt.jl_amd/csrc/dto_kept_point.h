// dto_kept_point.h -- the host half of a KEPT POINT: what an operator built at one point (Z [, sigma] [, mu]) and may use again at the
// same point, as ONE record.  Plain C++ (no HIP header, no engine header): tests/test_kept_point_header.py builds it with g++ alone.
// It decides what can be decided without the device; the copies of Z and mu and their bit compare are the device half (DevicePoint
// in dto_handle.h; at_kept_point, whose miss is the one caller of begin_rebuild, and keep_point in dto_engine.cpp).
//   key:     the handle's generation counter (dto_set_option, dto_set_external and every failed call bump it), and the parts named
//            at construction -- a TAG (int32), SIGMA (compared by its 64 bits: 0.0 and -0.0 are two points, a NaN equals itself),
//            the mark "mu was absent" (MU_MARK).  An argument that belongs to a part not named is ignored.
//   reading: may_hit(key) -- something is kept and every host-side part of the key matches.
//   writing: begin_rebuild() drops the record; keep(key) marks it kept, and ONLY between a begin_rebuild() and the next drop(): a
//            rebuild that throws between the two leaves nothing kept, and a keep() without a rebuild does nothing.
#pragma once

#include <cstdint>
#include <cstring>

namespace dto {

class KeptPoint {
public:
    enum : unsigned { TAG = 1, SIGMA = 2, MU_MARK = 4 };
    explicit KeptPoint(unsigned parts = 0) : parts_(parts) {}
    void drop() { state_ = DROPPED; }
    bool may_hit(uint64_t gen, int32_t tag, double sigma, bool mu_absent) const {
        return state_ == KEPT && gen == gen_ && (!(parts_ & TAG) || tag == tag_) &&
               (!(parts_ & SIGMA) || std::memcmp(&sigma, &sigma_, sizeof(double)) == 0) && (!(parts_ & MU_MARK) || mu_absent == mu_absent_);
    }
    void begin_rebuild() { state_ = REBUILDING; }
    void keep(uint64_t gen, int32_t tag, double sigma, bool mu_absent) {
        if (state_ != REBUILDING) return;
        gen_ = gen; tag_ = tag; sigma_ = sigma; mu_absent_ = mu_absent; state_ = KEPT;
    }

private:
    enum State { DROPPED, REBUILDING, KEPT };
    unsigned parts_;
    State state_ = DROPPED;
    uint64_t gen_ = 0;   // the key it was kept at
    int32_t tag_ = 0;
    double sigma_ = 0.0;
    bool mu_absent_ = false;
};

}  // namespace dto
