// The gradient ledger of one training step: everything the backward knows about a tensor, keyed by its device address.
//
// Two record kinds, because there are two key spaces.  An ActRec belongs to an ACTIVATION (its address is unique within a
// step: the training forward never recycles workspace): its gradient buffer, what its gradient is still owed, its flags,
// its operand twins.  A BufRec belongs to a device BUFFER that carries a tag (a two-byte tensor, a gradient buffer the
// side stream reads, ...): buffers include temporaries, whose addresses ARE handed out again, so release() drops the
// records of everything at or above the mark the workspace is rewound to.
//
// Host-only, plain C++17, no HIP header (a bf16 twin is held as void*): tests/grad_ledger_check.cpp runs it under the
// host compiler's sanitizers.
#pragma once
#include <stddef.h>

#include <algorithm>
#include <functional>
#include <unordered_map>
#include <utility>
#include <vector>

namespace sty {

// ---- what an activation's gradient buffer can still be owed (settled by whoever asks for the buffer first) ----
enum : unsigned {
  OWED_UP = 1,    // a pooled shortcut gradient that has still to be up-sampled into it
  OWED_ROW = 2,   // the row term coef[b][c] * act (the GRN term)
  OWED_GATE = 4,  // the factor lrelu'(act): the input-gradient conv wrote its raw output
  OWED_MASK = 8,  // its values altogether: the copy src * mask
};
struct PendUp {
  const float* g;     // [BC][H / 2][(W + 1) / 2 + 1]
  const float* mask;  // [B][n]: the mask of the activation's producer
  float scale;
  int BC, C, H, W, n;
};
struct PendRow {
  const float* coef;
  int rows, T;
};
struct PendGate {
  int C, n;  // channels, positions
};
struct LazyMask {
  const float* src;
  const float* mask;
  int C, n;
  float* dst;
};
// the instance norm a folded AdaIN scale `a` came from; done: the conv that consumes (a, s) ran the fused prologue +
// statistics backward, adain()'s own tape entry has nothing left to do
struct AdainInfo {
  const float *x, *s, *mean, *rstd, *gbl;
  float* dgl;
  bool done;
};

struct ActRec {
  float* g = nullptr;  // the gradient buffer (has_g: there is one; assigned by the G family of the tape alone)
  bool has_g = false;
  bool nograd = false;       // nobody wants this gradient
  bool reads_twin = false;      // its producer's backward reads the gradient as a bf16 twin
  bool twin_alone = false;  // ... and as the twin alone
  bool grad16 = false;       // its producer reads a two-byte gradient buffer
  bool has_adain = false;
  unsigned owed = 0;  // OWED_* bits; a term below is meaningful while its bit is set
  PendUp up;
  PendRow row;
  PendGate gate;
  LazyMask mask;
  void* twin[2] = {nullptr, nullptr};  // bf16(pro(x)) for pro = none, LeakyReLU
  AdainInfo adain;                     // keyed by the folded scale a
};

struct BufRec {
  bool half = false;       // two bytes per element behind a float* handle
  bool side_read = false;  // a side-stream launch reads it: never written again (copy on write)
  bool no_fp32 = false;    // a gradient whose one writer stored the twin and left the fp32 values out
  void* g16 = nullptr;     // its bf16 twin ...
  const float* g16_mask = nullptr;  // ... and the [B][n] mask the twin was multiplied by
  bool blank() const { return !half && !side_read && !no_fp32 && !g16; }
};

class GradLedger {
 public:
  // ---- activations ----
  ActRec& act(const void* p) { return acts_.try_emplace(p).first->second; }  // find or create; the reference stays valid
  ActRec* find_act(const void* p) {
    if (acts_.empty()) return nullptr;
    auto it = acts_.find(p);
    return it == acts_.end() ? nullptr : &it->second;
  }
  const ActRec* find_act(const void* p) const { return const_cast<GradLedger*>(this)->find_act(p); }
  // record that p's gradient is owed `kind`; the caller fills the term
  ActRec& owe(const void* p, unsigned kind) {
    ActRec& r = act(p);
    r.owed |= kind;
    owed_log_.emplace_back(p, kind);
    return r;
  }
  // the term is the caller's now: true once per owe()
  static bool take(ActRec& r, unsigned kind) {
    if (!(r.owed & kind)) return false;
    r.owed &= ~kind;
    return true;
  }
  // f(address, record) for every activation still owed `kind`, in the order the terms were recorded (f may record more)
  template <typename F>
  void each_owed(unsigned kind, F&& f) {
    for (size_t i = 0; i < owed_log_.size(); ++i) {
      const std::pair<const void*, unsigned> e = owed_log_[i];
      if (!(e.second & kind)) continue;
      ActRec* r = find_act(e.first);
      if (r && (r->owed & kind)) f(e.first, *r);
    }
  }

  // ---- buffers: sorted by address.  The workspace grows between two rewinds, so a new tag is nearly always appended ----
  BufRec& buf(const void* p) {  // find or create; valid until the next buf() / release()
    auto it = lower(p);
    if (it == bufs_.end() || it->first != p) it = bufs_.insert(it, std::make_pair(p, BufRec()));
    return it->second;
  }
  const BufRec* find_buf(const void* p) const {
    if (bufs_.empty()) return nullptr;
    auto it = const_cast<GradLedger*>(this)->lower(p);
    return it != bufs_.end() && it->first == p ? &it->second : nullptr;
  }
  void tag_half(const void* p) {
    BufRec& b = buf(p);
    n16_ += !b.half;
    b.half = true;
  }
  void tag_side_read(const void* p) {
    BufRec& b = buf(p);
    nside_ += !b.side_read;
    b.side_read = true;
  }
  // (fp32 mode asks on every conv launch: a test of a counter while nothing is tagged)
  bool is16(const void* p) const {
    if (!p || !n16_) return false;
    const BufRec* b = find_buf(p);
    return b && b->half;
  }
  bool any_side_reads() const { return nside_ != 0; }
  bool side_read(const void* p) const {
    if (!nside_) return false;
    const BufRec* b = find_buf(p);
    return b && b->side_read;
  }
  // the workspace is rewound to lo: every address at or above it is handed out again, without its tags
  void release(const void* lo) {
    if (bufs_.empty() || below(bufs_.back().first, lo)) return;
    auto it = lower(lo);
    for (auto j = it; j != bufs_.end(); ++j) {
      n16_ -= j->second.half;
      nside_ -= j->second.side_read;
    }
    bufs_.erase(it, bufs_.end());
  }
  void clear_side_reads() {
    if (!nside_) return;
    for (auto& e : bufs_) e.second.side_read = false;
    bufs_.erase(std::remove_if(bufs_.begin(), bufs_.end(), [](const Entry& e) { return e.second.blank(); }), bufs_.end());
    nside_ = 0;
  }

  void reset() {
    acts_.clear();
    bufs_.clear();
    owed_log_.clear();
    n16_ = nside_ = 0;
  }
  size_t n_acts() const { return acts_.size(); }
  size_t n_bufs() const { return bufs_.size(); }

 private:
  using Entry = std::pair<const void*, BufRec>;
  std::vector<Entry>::iterator lower(const void* p) {
    return std::lower_bound(bufs_.begin(), bufs_.end(), p, [](const Entry& e, const void* q) { return below(e.first, q); });
  }
  static bool below(const void* a, const void* b) { return std::less<const void*>()(a, b); }
  std::unordered_map<const void*, ActRec> acts_;  // node-based: a record's address holds across a rehash
  std::vector<Entry> bufs_;
  std::vector<std::pair<const void*, unsigned>> owed_log_;
  size_t n16_ = 0, nside_ = 0;
};

}  // namespace sty
