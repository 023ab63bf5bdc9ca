// The training tape: what every training graph of train.hip records its forward on and runs its backward from.  Nothing
// here knows a layer or a model.
//
// Each forward op pushes one closure; run_tape() runs them in reverse.  Gradient buffers are zero-filled when first
// requested (G) and every backward kernel accumulates, which makes fan-out (residual streams) trivial; a producer that
// can overwrite asks with Gw and the first writer skips the zero-fill.  What the backward knows about a tensor -- its
// gradient buffer, the terms that buffer is still owed, its bf16 twins, the tags of a buffer -- is one record in the
// ledger (grad_ledger.h); the G family below is the only code that assigns a record's gradient buffer, settle() the only
// place where owed terms are paid, release() the only rewind of the workspace.
//
// Every entry point follows one protocol.  Forward: open() binds stream, shape and workspace (or the fake base of a
// sizing pass), the graph's method records ops and tape, the outputs are copied out, and close_forward() reports the size
// (after a dry backward) or an overflow.  Backward: run_tape() seeds the output gradients, walks the tape in reverse,
// joins the weight-gradient stream and runs what the graph wants behind the join; close_backward() reports an overflow.
#pragma once
#include <stdlib.h>

#include <functional>
#include <vector>

#include "grad_ledger.h"
#include "model.h"

namespace sty {

struct Tape {
  // ---- the step ----
  sty_model* m = nullptr;
  hipStream_t st = nullptr;
  int B = 0, T = 0;
  Bump ws;
  int rc = STY_OK;
  size_t peak = 0;
  bool dry = false;  // sizing pass: fake base pointer, allocations are tracked but nothing is launched
  // deterministic mode (sty_set_deterministic), latched by open(): the forward, its sizing pass and the backward of that
  // forward all see this value, whatever the switch says by the time the backward runs
  bool det = false;
  std::vector<std::function<void()>> tape;
  GradLedger ledger;
  float* scratch_param = nullptr;  // sink for gradients of parameters nobody bound a gradient for
  size_t scratch_param_n = 0;
  // a tape entry gives its temporaries back -- unless it belongs to the prior branch's backward running beside the main stream
  // (keep_temps): the main stream's later entries would be handed the addresses while the branch's kernels still use them
  bool keep_temps = false;
  // ---- the prior branch of the vocoder graph (see Trainer::forward): where its resblocks run this step (nullptr: the main
  // stream; kept from the forward for the backward), its tape entries [branch_lo, branch_hi) and the entry of the conv it joins
  // the trunk at ----
  hipStream_t branch_st = nullptr;
  bool branch_can_beside = false;  // the graph takes a style stream (its workspace is sized without one)
  size_t branch_lo = 0, branch_hi = 0, branch_join = 0;
  // ---- side stream for the weight gradients (see below) ----
  hipStream_t st2 = nullptr;
  bool side_on = getenv("STY_NO_SIDE_STREAM") == nullptr;
  std::vector<hipEvent_t> evs;
  size_t ev_used = 0;
  bool side_dirty = false;
  size_t side_need = 0;  // floats
  float* side_partial = nullptr;
  // ---- deferred, grouped reduction of the weight-gradient partial sums (see below) ----
  WgReduceDefer* defer = wgrad_defer_create();
  bool defer_on = getenv("STY_NO_DEFERRED_REDUCE") == nullptr;
  size_t wg_sum = 0, wg_off = 0;  // floats
  float* wg_base = nullptr;
  int flush_site = 0;
  std::vector<std::function<void(hipStream_t)>> after_reduce;
  // ---- bf16 operand twins and two-byte storage (bf16 compute mode) ----
  bool twins_env = getenv("STY_NO_TWINS") == nullptr;
  bool act16_env = getenv("STY_NO_ACT16") == nullptr;

  ~Tape() {
    wgrad_defer_destroy(defer);
    for (hipEvent_t e : evs) (void)hipEventDestroy(e);
    if (st2) (void)hipStreamDestroy(st2);
  }

  bool live() const { return !dry && ws.base != nullptr && rc == STY_OK; }
  void chk(int r) {
    if (rc == STY_OK && r != STY_OK) rc = r;
  }
  // ---- the entry-point protocol: open, record the graph, close; backward = seed, tape, join (run_tape) ----
  // the sizing pass bumps from a fake base that is never dereferenced, under a cap no graph reaches
  static constexpr size_t kDryBase = size_t(1) << 30, kDryCap = size_t(1) << 46;
  // what a sizing pass adds to the measured peak
  static constexpr size_t kSlack = 64 << 20, kSlackStyle = 16 << 20;
  void open(int B_, int T_, void* ws_, size_t ws_bytes, hipStream_t st_, bool dry_) {
    st = st_;
    B = B_;
    T = T_;
    rc = STY_OK;
    ws = Bump();
    dry = dry_;
    det = deterministic_mode();
    ws.base = dry ? reinterpret_cast<char*>(kDryBase) : (char*)ws_;
    ws.cap = dry ? kDryCap : ws_bytes;
    peak = 0;
  }
  // the per-step state of the tape; everything per tensor is in the ledger
  void reset_step() {
    tape.clear();
    ledger.reset();
    side_need = 0;
    wg_sum = 0;
    branch_st = nullptr;
    branch_can_beside = false;
    branch_lo = branch_hi = branch_join = 0;
  }
  // the sizing pass (the entry has run its backward dry by now) reports the peak and drops the tape; the live pass reports
  // an overflow of the caller's workspace
  int close_forward(size_t* need, size_t ws_bytes, size_t slack, const char* what) {
    if (need) {
      *need = align_up(peak, 256) + slack;
      tape.clear();
      return rc;
    }
    if (ws.overflow) {
      set_error("%s workspace too small: need %zu bytes, have %zu", what, peak, ws_bytes);
      return STY_ENOMEM;
    }
    return rc;
  }
  int close_backward() {
    if (ws.overflow) {
      set_error("training workspace too small in backward: need %zu bytes", peak);
      return STY_ENOMEM;
    }
    return rc;
  }
  void copy_f32(float* dst, const float* src, size_t n, const char* what) {  // device to device, on the main stream
    if (!live()) return;
    hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) rc = hip_fail(e, what);
  }
  // the gradient buffer of a graph output, holding the caller's gradient d (sizing pass: d == nullptr, the buffer alone)
  float* seed(const float* act, const float* d, size_t n) {
    float* g = G(act, n);
    if (d) copy_f32(g, d, n, "seed copy");
    return g;
  }
  // The backward of every graph.  `seeds` calls seed() for each output; the tape runs in reverse and stops at the first
  // error.  flush_up (the style encoders): pooled shortcut gradients nobody has asked for are up-sampled before the join.
  // after_join (every graph with AdaIN / AdaLN layers: fc(style)'s backward) runs behind the join of the side stream.
  void run_tape(const std::function<void()>& seeds, bool flush_up, const std::function<void()>& after_join) {
    side_begin();
    seeds();
    // The prior branch's entries [branch_lo, branch_hi) need nothing but G(lap) / G(pp), which the entry
    // branch_join (phase_input_conv) writes, and nothing on the main stream needs them before fc(style)'s backward: with a
    // branch stream they are issued there as soon as branch_join has run, in their own reverse order, and skipped at their place,
    // where the main stream waits for their end instead.  The sizing pass of a graph that can be given a style stream (the speech
    // graph: branch_can_beside) always walks the tape in that order (the larger need).
    const bool br = branch_lo < branch_hi && branch_hi <= branch_join && branch_join < tape.size();
    const bool br_beside = br && (branch_st || (dry && branch_can_beside));
    hipEvent_t br_end = nullptr;
    for (size_t i = tape.size(); i-- > 0 && rc == STY_OK;) {
      if (br_beside && i >= branch_lo && i < branch_hi) {
        if (i + 1 == branch_hi && br_end) {
          hipError_t r = hipStreamWaitEvent(st, br_end, 0);
          if (r != hipSuccess) rc = hip_fail(r, "prior branch backward join");
          br_end = nullptr;
        }
        continue;
      }
      tape[i]();
      if (rc != STY_OK || !br_beside || i != branch_join) continue;
      hipStream_t const main_st = st;
      if (branch_st) {
        stream_after(branch_st, main_st, "prior branch backward fork");
        st = branch_st;  // side_push, fresh_copy, the zero-fills of G and every launch of the entries follow
      }
      keep_temps = true;
      for (size_t j = branch_hi; j-- > branch_lo && rc == STY_OK;) tape[j]();
      keep_temps = false;
      st = main_st;
      if (branch_st && live()) {  // (also behind an entry that failed: what it did issue is joined below)
        const int rc0 = rc;
        rc = STY_OK;
        br_end = next_event();
        if (rc == STY_OK && hipEventRecord(br_end, branch_st) != hipSuccess) {
          br_end = nullptr;
          rc = hip_fail(hipGetLastError(), "prior branch backward end");
        }
        if (rc0 != STY_OK) rc = rc0;
      }
    }
    // an error left the loop before the branch's place: the caller's style stream is joined all the same
    if (br_end) (void)hipStreamWaitEvent(st, br_end, 0);
    // terms nobody asked for, in the order they were recorded (each pass writes a buffer of its own)
    if (flush_up)
      ledger.each_owed(OWED_UP, [this](const void* a, ActRec& r) {
        if (rc == STY_OK) up_flush(static_cast<const float*>(a), r);
      });
    ledger.each_owed(OWED_ROW, [this](const void* a, ActRec& r) {
      if (rc == STY_OK) row_flush(static_cast<const float*>(a), r);
    });
    side_join();
    if (after_join && rc == STY_OK) after_join();
  }

  // ---- events ----
  hipEvent_t next_event() {
    if (ev_used == evs.size()) {
      hipEvent_t e = nullptr;
      hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
      if (r != hipSuccess) rc = hip_fail(r, "event");
      evs.push_back(e);
    }
    return evs[ev_used++];
  }
  // `to` waits for what `from` holds so far
  void stream_after(hipStream_t to, hipStream_t from, const char* what) {
    if (!live() || rc != STY_OK) return;
    hipEvent_t e = next_event();  // (the pool is reset at the start of the backward; the forward's events come behind its last)
    if (rc != STY_OK) return;
    hipError_t r = hipEventRecord(e, from);
    if (r == hipSuccess) r = hipStreamWaitEvent(to, e, 0);
    if (r != hipSuccess) rc = hip_fail(r, what);
  }

  // ---- side stream for the weight gradients ----
  // A weight gradient is a leaf of the backward graph: it reads (x, gY) and nothing reads it before the optimizer.
  // On the sample_dataset shapes the input-gradient chain is a sequence of kernels too small to fill 256 CUs, so the
  // weight-gradient kernels (512-1024 workgroups each) run on a second, lower-priority stream and take the idle CUs.
  // Each launch is handed over at once (one event on the main stream per launch; measured against batches of launches:
  // c2 step 46.9 ms at 1, 47.5 at 4, 49.0 at 16: the weight gradient then
  // overlaps the input gradient of its own layer, a kernel of the same size class).  The side stream only ever waits for the main
  // stream; the main stream never waits for the side stream before the join at the end of the tape, because a
  // gradient buffer with a side-stream reader is never written again: when G / Gw find such a buffer (BufRec::side_read; it can
  // only be written again through the residual aliasing) they hand out a copy instead (copy on write).
  // The side stream has its own partial-sum buffer (side_partial, sized in the forward for the largest conv): the
  // main stream recycles its temporaries while the side-stream launches are still pending.
  void side_begin() {
    ev_used = 0;
    ledger.clear_side_reads();
    side_dirty = false;
    const bool on = side_on && !single_stream_mode();
    side_partial = on && side_need ? take<float>(side_need) : nullptr;
    wg_base = defer_on && wg_sum ? take<float>(wg_sum) : nullptr;
    wg_off = 0;
    flush_site = 0;
    after_reduce.clear();
    if (on && !st2 && live()) {
      // (Measured and rejected: hipExtStreamCreateWithCUMask leaving every 2nd / 4th / 8th CU to the main stream, so
      // that its small kernels need not wait for a resident weight-gradient workgroup to retire -- c2 38.0 -> 62 ms,
      // c3 120.5 -> 144.5 ms at every mask: masked streams lose far more than the waiting costs.)
      int least = 0, greatest = 0;
      (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
      hipError_t r = hipStreamCreateWithPriority(&st2, hipStreamNonBlocking, least);
      if (r != hipSuccess) rc = hip_fail(r, "side stream");
    }
  }
  bool side_ready() const { return side_partial != nullptr; }  // also in the sizing pass (same allocations)
  // launch on the side stream, behind the main stream's work so far, what reads gbuf (complete on the main stream at this
  // point) and nothing the main stream writes later
  void side_push(const float* gbuf, const std::function<void(hipStream_t)>& fn) {
    ledger.tag_side_read(gbuf);
    if (!live() || !st2) return;
    hipEvent_t e = next_event();
    if (rc == STY_OK) {
      hipError_t r = hipEventRecord(e, st);
      if (r == hipSuccess) r = hipStreamWaitEvent(st2, e, 0);
      if (r != hipSuccess) rc = hip_fail(r, "side fork");
    }
    if (rc == STY_OK) {
      DeferScope ds(this);
      fn(st2);
    }
    side_dirty = true;
  }
  void side_reduce_nowait() {
    if (side_dirty && st2) reduce_flush(st2);
  }
  void side_join() {
    reduce_flush(side_dirty && st2 ? st2 : st);
    if (side_dirty && st2) {
      hipEvent_t e = next_event();
      hipError_t r = hipEventRecord(e, st2);
      if (r == hipSuccess) r = hipStreamWaitEvent(st, e, 0);
      if (r != hipSuccess) rc = hip_fail(r, "side join");
    }
    ledger.clear_side_reads();
    side_dirty = false;
  }
  // ---- deferred, grouped reduction of the weight-gradient partial sums (wgrad.hip) ----
  // Every weight-gradient launch of a backward gets a partial buffer of its own (wg_take, out of one region sized in the
  // forward: wg_sum), its reduction is recorded instead of launched, and reduce_flush sums everything recorded so far in
  // one launch on the stream the weight gradients run on -- before a gradient segment is announced and at the end of the
  // backward -- followed by the few steps that READ a reduced gradient (`after_reduce`: d alpha of the lean ConvNeXt32
  // backward is a function of dW1).
  bool deferring() const { return wg_base != nullptr; }
  float* wg_take(size_t n) {
    n = (n + 63) & ~size_t(63);
    float* p = wg_base + wg_off;
    wg_off += n;
    if (wg_off > wg_sum && rc == STY_OK) {
      set_error("training: weight-gradient partial region too small (%zu > %zu floats)", wg_off, wg_sum);
      rc = STY_ESTATE;
    }
    return p;
  }
  void wg_need(size_t n) { wg_sum += (n + 63) & ~size_t(63); }
  struct DeferScope {  // the defer context is current on this thread while a backward issues launches
    WgReduceDefer* old;
    explicit DeferScope(Tape* t) { old = wgrad_defer_set(t->deferring() && t->live() ? t->defer : nullptr); }
    ~DeferScope() { (void)wgrad_defer_set(old); }
  };
  void reduce_flush(hipStream_t s) {
    if (!deferring() || !live()) {
      after_reduce.clear();
      return;
    }
    // deterministic mode: the partial slots summed here (det_sum) were written on the main stream, after the side stream's
    // last wait for it
    if (det && s != st) stream_after(s, st, "deterministic partials");
    chk(wgrad_defer_flush(defer, flush_site++, s));
    WgReduceDefer* cur = wgrad_defer_set(nullptr);  // (what runs now reduces at once, should it reduce at all)
    if (rc == STY_OK)
      for (auto& fn : after_reduce) fn(s);
    (void)wgrad_defer_set(cur);
    after_reduce.clear();
  }

  // ---- deterministic mode: batch-summed parameter gradients without atomics ----
  // det_slots: a [slots][n] partial buffer for a launcher's `det` form, or nullptr (default mode / no gradient wanted).  It has
  // to outlive the entry that takes it (the grouped reduction reads it at the next flush), so an entry takes it BEFORE its
  // mark; the sizing pass walks the same code, so the workspace figure of the mode includes every such buffer.
  // det_sum: out[i] += sum_k part[k][i], k in index order -- recorded into the grouped reduction of the weight gradients
  // where one is deferring (no launch of its own; jobs onto one destination go to consecutive rounds in recording order),
  // launched at once on the main stream otherwise or when `now` (somebody reads `out` before the next flush).
  // (a gradient nobody bound goes to the scratch sink: it keeps the atomic form -- its values are never read, and reduce jobs
  // onto the one sink would all overlap, each in a round and a launch of its own)
  float* det_slots(const float* grad, size_t slots, size_t n) {
    return det && grad && grad != scratch_param ? take<float>(slots * n) : nullptr;
  }
  void det_sum(const float* part, size_t slots, size_t n, float* out, bool now = false) {
    if (!part || !live()) return;
    if (now) {
      WgReduceDefer* cur = wgrad_defer_set(nullptr);
      launch_wgrad_reduce_planes(part, (int)slots, n, n, 0, out, nullptr, st);
      (void)wgrad_defer_set(cur);
    } else {
      DeferScope ds(this);
      launch_wgrad_reduce_planes(part, (int)slots, n, n, 0, out, nullptr, st);
    }
  }
  // ---- workspace ----
  template <typename Tp>
  Tp* take(size_t n) {
    Tp* p = ws.take<Tp>(n);
    peak = ws.off > peak ? ws.off : peak;
    return p;
  }
  // THE rewind: a tape entry gives back what it took since `mark` (= ws.off then), and the tags of those buffers go with
  // them -- the addresses are handed out again, possibly to a tensor of another kind.  Not while keep_temps holds (above).
  void release(size_t mark) {
    if (keep_temps) return;
    ws.off = mark;
    ledger.release(ws.base + mark);
  }
  // ---- bf16 STORAGE of the 75T-rate activations (bf16 compute mode) ----
  // What autocast stores: conv outputs live in HBM as bf16 (config/config.yml:9-12, train/train_context.py:97-103).  A tensor
  // taken with take_act(n, true) IS two bytes per element -- there is no fp32 copy -- and travels through the graph as an
  // opaque `float*` handle; BufRec::half records which handles are such tensors and every launch site passes the flag of each
  // operand (ConvArgs::xh / yh / rh, the uh / xh / dh arguments of the element-wise kernels).  Kernels that have no
  // two-byte form refuse the flag loudly (launch_conv1d, launch_conv1d_wgrad).  Gradient ACCUMULATORS (G / Gw buffers)
  // stay fp32: they are summed into by several kernels, and the rounding points of the mode stay those of single stores.
  bool act16_on() const { return act16_env && m->topts.compute_bf16 != 0; }
  bool is16(const void* p) const { return ledger.is16(p); }
  float* take_act(size_t n, bool h) {
    if (!h) return take<float>(n);
    float* p = reinterpret_cast<float*>(take<__bf16>((n + 7) & ~size_t(7)));
    ledger.tag_half(p);
    return p;
  }
  // ---- bf16 operand twins (ConvArgs::x16 / g16; bf16 compute mode) ----
  // ActRec::twin[pro]: the twin bf16(pro(x)) of an activation (pro = PRO_NONE, PRO_LRELU), written by the kernel that produced
  // the activation where that kernel has the output stage for it, by the cast pass (launch_twin_cast) otherwise; kept to the
  // end of the step (the forward conv reads it, the weight gradient reads it again in the backward).
  // Gradient twins: ActRec::reads_twin = an activation y whose conv will read G(y) as a twin (its weight gradient runs on
  // wgradb16); BufRec::g16 / g16_mask = the twin of a gradient buffer and the [B][n] mask it was multiplied by, registered by
  // the element-wise backward kernel that writes the buffer LAST (pooling / learned down-sampling backward); the conv's
  // backward takes it when the mask is its own, and makes the twin with the cast pass otherwise.
  // Gradient stores nobody loads (style encoder, twins on): ActRec::twin_alone = a conv output y whose conv reads G(y) through
  // the twin alone (conv2d decides with bwd_reads_twin_only when it records the conv); the element-wise backward that is the
  // one writer of such a gradient then stores the twin and leaves the fp32 tensor out (dwconv2d_s2_bwd: conv1 of a
  // down-sampling ResBlk), and the buffer is tagged BufRec::no_fp32: conv2d_bwd refuses one it would have to load.
  bool twins_on() const { return twins_env && m->topts.compute_bf16 != 0; }
  static int tw_slot(int pro) { return pro == PRO_LRELU ? 1 : 0; }
  void twin_register(const float* x, int pro, __bf16* t) { ledger.act(x).twin[tw_slot(pro)] = t; }
  const __bf16* xtwin(const float* x, int pro, int C, int n) {
    void*& slot = ledger.act(x).twin[tw_slot(pro)];
    if (!slot) {
      __bf16* t = take<__bf16>((size_t)B * C * n);
      if (live()) chk(launch_twin_cast(x, nullptr, pro, B, C, n, t, st));
      slot = t;
    }
    return static_cast<const __bf16*>(slot);
  }
  void set_grad_twin(const float* g, const __bf16* g16, const float* mask) {
    BufRec& b = ledger.buf(g);
    b.g16 = const_cast<__bf16*>(g16);
    b.g16_mask = mask;
  }

  // ---- the gradient buffers ----
  bool wants(const float* act) const {
    const ActRec* r = ledger.find_act(act);
    return !(r && r->nograd);
  }
  void no_grad(const float* act) { ledger.act(act).nograd = true; }
  bool has_grad(const float* act) const {
    const ActRec* r = ledger.find_act(act);
    return r && r->has_g;
  }
  float* bind(ActRec& r, float* g) {
    r.g = g;
    r.has_g = true;
    return g;
  }
  // Owed terms, paid in this order before anybody gets the buffer.  `keep`: the kinds the caller deals with itself.
  // `writer` (Gw): a second writer -- the buffer of a pending masked copy gets its values now, and the twin it shared with
  // the copy's source is no longer its twin.
  //   up:   the pooled gradient of a shortcut branch that has still to be up-sampled into G(x) (the backward of pool(x)).  The
  //         branch's backward runs BEFORE the main branch's first conv (style_forward records them in that order); that conv's
  //         input-gradient conv then takes the pooled gradient as an output-stage operand (ConvArgs::up_g: gate, up-sample and
  //         twin in its epilogue) where the kernel has the stage, and the element-wise pass (up_apply: what the tape entry of
  //         pool() used to launch) runs behind it otherwise -- or for whoever else asks for G(x) first.
  //   row:  the row term coef[b][c] * h (the GRN term of convnext()): the activation backward of act() forms it in registers
  //         on its way (take_row); anybody else gets the plain pass.
  //   gate: deferred LeakyReLU gates (style encoder): the buffer still lacks the factor lrelu'(a) -- the input-gradient conv
  //         of a LeakyReLU-prologue conv wrote its raw output there (conv2d_bwd).  The next element-wise step that touches the
  //         buffer anyway applies the factor on its way (avgpool2_bwd accumulating into it, dwconv2d_s2_bwd reading it);
  //         anybody else gets the plain pass first.
  //   mask: the copy `G(act) = src * mask`: the shortcut branch's gradient is the block's output gradient times the output
  //         mask, which the twin g16 already holds value for value.  The copy is made for whoever asks for the fp32 buffer,
  //         and never when the one reader takes the twin.
  void settle(const float* act, ActRec& r, unsigned keep, bool writer) {
    if (r.owed & OWED_UP) up_flush(act, r);
    if (r.owed & OWED_ROW & ~keep) row_flush(act, r);
    if (r.owed & OWED_GATE & ~keep) gate_flush(act, r);
    if (r.owed & OWED_MASK & ~keep) {
      if (writer) set_grad_twin(r.mask.dst, nullptr, nullptr);
      mask_flush(act, r);
    }
  }
  void up_apply(const float* src, const PendUp& u) {
    // gs = gs * lrelu'(src) + up(g) in the one pass that accumulates into gs anyway
    ActRec& r = ledger.act(src);
    const bool gated = ledger.take(r, OWED_GATE);
    float* gs = G(src, (size_t)u.BC * u.n);
    // this pass is the last writer of d loss / d src: it also leaves the bf16 operand twin for src's producer
    __bf16* g16 = twins_on() && r.reads_twin && u.n % 4 == 0 ? take<__bf16>((size_t)u.BC * u.n) : nullptr;
    if (g16) set_grad_twin(gs, g16, u.mask);
    if (live()) chk(launch_avgpool2_bwd(u.g, u.BC, u.H, u.W, u.scale, gs, gated ? src : nullptr, st, g16, u.mask, u.C));
  }
  void up_flush(const float* act, ActRec& r) {
    if (ledger.take(r, OWED_UP)) up_apply(act, PendUp(r.up));
  }
  void row_flush(const float* act, ActRec& r) {
    if (!ledger.take(r, OWED_ROW)) return;
    const PendRow p = r.row;
    float* g = G(act, (size_t)p.rows * p.T);  // (the term is taken: no way back here)
    if (live()) chk(launch_row_scale_add(act, p.coef, 0.f, p.rows, p.T, g, st));
  }
  const float* take_row(const float* act) {  // the pending term's coefficients (nullptr: none); the caller applies it
    ActRec* r = ledger.find_act(act);
    return r && ledger.take(*r, OWED_ROW) ? r->row.coef : nullptr;
  }
  bool gate_pending(const float* act) const {
    const ActRec* r = ledger.find_act(act);
    return r && (r->owed & OWED_GATE);
  }
  void gate_flush(const float* act, ActRec& r) {
    if (!ledger.take(r, OWED_GATE) || !r.has_g || !live()) return;
    float* g = r.g;  // in place: one element per thread, read then written
    chk(launch_pro_bwd(PRO_LRELU, g, r.gate.C, 0, act, B, r.gate.C, r.gate.n, nullptr, nullptr, r.gate.C, 0, nullptr, nullptr, g,
                       0, nullptr, nullptr, nullptr, st));
  }
  void mask_flush(const float* act, ActRec& r) {
    if (!ledger.take(r, OWED_MASK)) return;
    const LazyMask z = r.mask;
    if (live())
      chk(launch_pro_bwd(PRO_MASK, z.src, z.C, 0, z.src, B, z.C, z.n, nullptr, nullptr, z.C, 0, nullptr, z.mask, z.dst, 0,
                         nullptr, nullptr, nullptr, st));
  }
  // gradient buffer of an activation (zero-filled on first request)
  float* G(const float* act, size_t n, unsigned keep = 0) {
    ActRec& r = ledger.act(act);
    if (r.owed) settle(act, r, keep, false);
    if (r.has_g && is16(r.g)) {
      set_error("a two-byte gradient buffer reached a consumer without a two-byte form");
      rc = STY_ESTATE;
    }
    if (r.has_g) return side_cow(r, n);
    float* g = take<float>(n);
    if (live()) {
      hipError_t e = hipMemsetAsync(g, 0, n * sizeof(float), st);
      if (e != hipSuccess) rc = hip_fail(e, "grad memset");
    }
    return bind(r, g);
  }
  // same, for a producer that can either overwrite or accumulate: the first writer of a buffer overwrites it
  // (acc = 0) and no zero-fill is issued; later writers accumulate
  float* Gw(const float* act, size_t n, int& acc) {
    ActRec& r = ledger.act(act);
    if (r.owed) settle(act, r, 0, true);
    if (r.has_g && is16(r.g)) {
      set_error("a two-byte gradient buffer reached a second writer");
      rc = STY_ESTATE;
    }
    acc = r.has_g ? 1 : 0;
    return r.has_g ? side_cow(r, n) : bind(r, take<float>(n));
  }
  // the gradient buffer of `act` for a consumer that can read a two-byte one
  float* G16(const float* act, size_t n) {
    const ActRec* r = ledger.find_act(act);
    if (r && r->has_g && is16(r->g)) return r->g;
    return G(act, n);
  }
  // act's gradient gets a buffer of its own that the caller writes every element of (no zero-fill): the first and only
  // writer of a two-byte gradient (its reader takes bf16, each value is rounded once where it is stored; G / Gw refuse such a
  // buffer: nothing accumulates into it), or a kernel that rewrites out of place a buffer the side stream still reads
  float* fresh_grad(const float* act, size_t n, bool two_byte) { return bind(ledger.act(act), take_act(n, two_byte)); }
  // the gradient of `act` IS the buffer g (act has exactly one consumer, whose backward produced g in place): no zero-fill,
  // no accumulate pass.  false if act already has a gradient buffer (another consumer wrote first): the caller adds instead.
  bool alias_grad(const float* act, float* g) {
    ActRec& r = ledger.act(act);
    if (r.has_g) return false;
    bind(r, g);
    return true;
  }
  // copy on write of a gradient buffer the side stream reads
  float* side_cow(ActRec& r, size_t n) { return ledger.side_read(r.g) ? fresh_copy(r, n) : r.g; }
  float* fresh_copy(ActRec& r, size_t n) {
    float* g2 = take<float>(n);
    copy_f32(g2, r.g, n, "grad copy");
    return bind(r, g2);
  }

  // parameter gradient pointer: packed (inside the grad arena) or bound by the caller
  float* PGpacked(const float* packed) const {
    if (!packed || !m->garena) return nullptr;
    return reinterpret_cast<float*>(m->garena + (reinterpret_cast<const char*>(packed) - m->arena));
  }
  float* PG(const float* param, size_t n) {
    auto it = m->pgrad.find(param);
    if (it != m->pgrad.end()) return it->second;
    if (n > scratch_param_n) return nullptr;
    return scratch_param;
  }
};

}  // namespace sty
