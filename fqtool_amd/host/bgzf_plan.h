// bgzf_plan.h -- windows of a BGZF input for the raw stream's device inflate (FQ_GZ_IN_DEVICE=2).
//
// A pure function over the member chain that BgzfSource::walk collects (header only, no other
// dependency: tools/micro/bgzf_plan_sim.cpp runs it under AddressSanitizer).  The inflated stream is
// cut into windows [S, L) that are whole numbers of the reference's gzread calls (`call` bytes,
// 1 MiB: src/fqreader.cpp:28-35): S is a multiple of call, L a call boundary or the stream's end.
// The reference's stream of a corrupt file ends at the start of the failing call, and a window is
// used only if all its members inflate, so everything the raw stream has taken lies at or before
// the S of the first bad window, which is at or before where the reference's stream ends: the host
// reader resumes there and zlib alone decides where the stream ends and what is reported.
//
// A window's members are those that hold its bytes: from the member that holds byte S (skip = S -
// that member's start: its leading bytes belong to the window before, where the member was checked
// too) to the member that holds byte L - 1, empty members between them, and the empty members at L
// (so every member of the file is inflated by some window; the last window's are the EOF members).
// What the engine needs of a window: at most member_cap members, the compressed range (first
// payload's start to last payload's end) and the inflated bytes from S to the last member's end
// both within `cap` bytes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cstddef>
#include <vector>

struct BgzfChainMember {
    uint64_t data;  // file offset of the deflate payload
    uint32_t clen;  // its length
    uint32_t isize;
    uint32_t crc;
};

struct BgzfWindowPlan {
    uint64_t start = 0, n = 0;       // the window: stream bytes [start, start + n)
    size_t first = 0, end = 0;       // its members [first, end)
    uint32_t skip = 0;               // start - (stream offset of member `first`)
    uint64_t comp_off = 0, comp_bytes = 0;  // file range of the members' payloads
};

class BgzfPlanner {
   public:
    BgzfPlanner(std::vector<BgzfChainMember> members, uint64_t call, uint64_t cap, uint32_t member_cap)
        : ms_(std::move(members)), call_(std::max<uint64_t>(call, 1)), cap_(cap), member_cap_(member_cap) {
        off_.reserve(ms_.size() + 1);
        uint64_t o = 0;
        for (const BgzfChainMember& m : ms_) {
            off_.push_back(o);
            o += m.isize;
        }
        off_.push_back(o);
    }
    uint64_t size() const { return off_.back(); }
    const std::vector<BgzfChainMember>& members() const { return ms_; }
    uint64_t member_start(size_t i) const { return off_[i]; }
    // every single call of the stream is a window the engine takes (then next() never fails)
    bool fits() const {
        if (cap_ < call_) return false;
        BgzfWindowPlan w;
        for (uint64_t s = 0; s < size(); s += call_)
            if (!span(s, std::min(size(), s + call_), w)) return false;
        return true;
    }
    // The window at S (a call multiple, or the stream's end) for a reader that wants `want` more
    // bytes: L = the first call boundary at or past S + want, but not beyond S + cap, or the stream's
    // end; shrunk by whole calls until the engine takes it.  want = 0 (or S at the end) gives the empty
    // window without members.  false: not even one call fits (fits() is false).
    bool next(uint64_t S, uint64_t want, BgzfWindowPlan& w) const {
        w = BgzfWindowPlan();
        w.start = S;
        if (want == 0 || S >= size()) return true;
        const uint64_t hi = S + cap_ >= size() ? size() : (S + cap_) / call_ * call_;
        uint64_t L = std::min(hi, (S + want + call_ - 1) / call_ * call_);
        L = std::min(L, size());
        for (;;) {
            if (L <= S) return false;
            if (span(S, L, w)) return true;
            // (the stream's end is not a call boundary: the first step back goes to the one before it)
            L = L % call_ ? L / call_ * call_ : L - call_;
        }
    }

   private:
    // the members of [S, L) into w; false if the engine would refuse them
    bool span(uint64_t S, uint64_t L, BgzfWindowPlan& w) const {
        // the member that holds byte x: the last one that starts at or before x and is not empty
        auto holder = [&](uint64_t x) { return (size_t)(std::upper_bound(off_.begin(), off_.end(), x) - off_.begin()) - 1; };
        const size_t first = holder(S);
        size_t end = holder(L - 1) + 1;
        while (end < ms_.size() && ms_[end].isize == 0 && off_[end] == L) ++end;
        if (L == size()) end = ms_.size();
        const uint64_t comp_off = ms_[first].data;
        const uint64_t comp_end = ms_[end - 1].data + ms_[end - 1].clen;
        if (end - first > member_cap_ || comp_end < comp_off || comp_end - comp_off > cap_ || off_[end] - S > cap_) return false;
        w.start = S;
        w.n = L - S;
        w.first = first;
        w.end = end;
        w.skip = (uint32_t)(S - off_[first]);
        w.comp_off = comp_off;
        w.comp_bytes = comp_end - comp_off;
        return true;
    }
    std::vector<BgzfChainMember> ms_;
    uint64_t call_, cap_;
    uint32_t member_cap_;
    std::vector<uint64_t> off_;  // stream offset of each member, then the stream's size
};
