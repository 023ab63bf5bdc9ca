// Stand-alone check of csrc/grad_ledger.h (host-only; tests/test_grad_ledger.py builds it with the host compiler's address
// and undefined-behaviour sanitizers and runs it).  Addresses are made up: the ledger never dereferences a key.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../stylish_tts_amd/csrc/grad_ledger.h"

using namespace sty;

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      ++failures;                                               \
    }                                                           \
  } while (0)

static const float* addr(uintptr_t a) { return reinterpret_cast<const float*>(a); }

int main() {
  const uintptr_t base = uintptr_t(1) << 30;
  // ---- buffer tags and the rewind ----
  {
    GradLedger L;
    CHECK(!L.is16(addr(base)) && !L.is16(nullptr) && !L.any_side_reads());
    L.tag_half(addr(base + 256));                // a persistent two-byte tensor below the mark
    L.tag_side_read(addr(base + 512));           // ... and a gradient buffer the side stream reads
    const uintptr_t mark = base + 1024;
    L.tag_half(addr(mark));                      // temporaries at and above the mark
    L.tag_half(addr(mark + 4096));
    L.tag_side_read(addr(mark + 2048));
    L.buf(addr(mark + 8192)).no_fp32 = true;
    L.tag_side_read(addr(base + 768));           // (tagged after the temporaries, below them)
    CHECK(L.is16(addr(mark)) && L.is16(addr(mark + 4096)) && !L.is16(addr(mark + 2048)));
    L.release(addr(mark));
    CHECK(!L.is16(addr(mark)) && !L.is16(addr(mark + 4096)));       // untagged after release(mark)
    CHECK(!L.side_read(addr(mark + 2048)) && !L.find_buf(addr(mark + 8192)));
    CHECK(L.is16(addr(base + 256)));                                // a tag below the mark survives
    CHECK(L.side_read(addr(base + 512)) && L.side_read(addr(base + 768)));
    CHECK(L.n_bufs() == 3);
    // the address is handed out again, to an fp32 tensor this time
    L.tag_side_read(addr(mark));
    CHECK(!L.is16(addr(mark)) && L.side_read(addr(mark)));
    L.release(addr(mark + 256));  // nothing at or above: nothing goes
    CHECK(L.side_read(addr(mark)) && L.n_bufs() == 4);
    // the gradient twin of a buffer
    BufRec& b = L.buf(addr(base + 512));
    int twin = 0;
    b.g16 = &twin;
    b.g16_mask = addr(base + 64);
    L.clear_side_reads();
    CHECK(!L.any_side_reads() && !L.side_read(addr(base + 512)) && !L.side_read(addr(mark)));
    CHECK(L.find_buf(addr(base + 512)) && L.find_buf(addr(base + 512))->g16 == &twin);  // the twin stays
    CHECK(!L.find_buf(addr(mark)) && !L.find_buf(addr(base + 768)));                      // records without a tag go
    CHECK(L.is16(addr(base + 256)));
    L.release(addr(base));
    CHECK(L.n_bufs() == 0 && !L.is16(addr(base + 256)));
  }
  // ---- owed terms: recording order, each kind taken once ----
  {
    GradLedger L;
    const int N = 40;
    for (int i = 0; i < N; ++i) {  // descending addresses: neither address order nor hash order is recording order
      const float* a = addr(base + (uintptr_t)(N - i) * 4096);
      L.owe(a, i % 2 ? OWED_ROW : OWED_UP);
      if (i % 2)
        L.act(a).row = PendRow{a, i, 1};
      else
        L.act(a).up = PendUp{a, nullptr, 1.f, i, 0, 0, 0, 0};
    }
    std::vector<int> seen;
    L.each_owed(OWED_UP, [&](const void* a, ActRec& r) {
      CHECK(r.up.g == a);
      seen.push_back(r.up.BC);
      CHECK(GradLedger::take(r, OWED_UP));
    });
    CHECK(seen.size() == N / 2);
    for (size_t k = 0; k < seen.size(); ++k) CHECK(seen[k] == (int)(2 * k));
    seen.clear();
    L.each_owed(OWED_UP, [&](const void*, ActRec&) { seen.push_back(0); });
    CHECK(seen.empty());  // all taken
    // a term taken in between is skipped; one recorded from inside the walk is reached
    ActRec* r3 = L.find_act(addr(base + (uintptr_t)(N - 3) * 4096));
    CHECK(r3 && GradLedger::take(*r3, OWED_ROW));
    const float* late = addr(base + 64);
    bool added = false;
    L.each_owed(OWED_ROW, [&](const void* a, ActRec& r) {
      seen.push_back(a == late ? -1 : r.row.rows);
      if (!added) {
        L.owe(late, OWED_ROW).row = PendRow{late, -1, 1};
        added = true;
      }
    });
    CHECK(seen.size() == N / 2);  // 20 rows, one taken, one added
    CHECK(seen.front() == 1 && seen[1] == 5 && seen.back() == -1);

    const float* a = addr(base + 128);
    const unsigned kinds[4] = {OWED_UP, OWED_ROW, OWED_GATE, OWED_MASK};
    for (unsigned k : kinds) L.owe(a, k);
    L.act(a).gate = PendGate{3, 7};
    L.act(a).mask = LazyMask{a, nullptr, 3, 7, nullptr};
    ActRec& r = L.act(a);
    CHECK(r.owed == (OWED_UP | OWED_ROW | OWED_GATE | OWED_MASK));
    for (unsigned k : kinds) {
      CHECK(GradLedger::take(r, k));
      CHECK(!GradLedger::take(r, k));  // exactly once
    }
    CHECK(r.owed == 0 && r.gate.C == 3 && r.mask.n == 7);
  }
  // ---- records stay where they are across a rehash; the adain flag through two lookups ----
  {
    GradLedger L;
    const float* a0 = addr(base + 8);
    ActRec* first = &L.act(a0);
    first->grad16 = true;
    first->adain = AdainInfo{a0, nullptr, nullptr, nullptr, nullptr, nullptr, false};
    first->has_adain = true;
    for (int i = 1; i <= 20000; ++i) L.act(addr(base + 8 + (uintptr_t)i * 256)).nograd = (i % 3 == 0);
    CHECK(L.n_acts() == 20001);
    CHECK(&L.act(a0) == first && L.find_act(a0) == first && first->grad16 && first->adain.x == a0);
    CHECK(L.find_act(addr(base + 8 + 256 * 3))->nograd && !L.find_act(addr(base + 8 + 256 * 4))->nograd);
    CHECK(!L.find_act(addr(base + 9)));
    L.act(a0).adain.done = true;  // set through one lookup ...
    const GradLedger& cL = L;
    CHECK(cL.find_act(a0)->adain.done && first->adain.done);  // ... seen through another
    // ---- reset ----
    L.tag_half(a0);
    L.tag_side_read(a0);
    L.owe(a0, OWED_GATE);
    L.reset();
    CHECK(L.n_acts() == 0 && L.n_bufs() == 0);
    CHECK(!L.is16(a0) && !L.any_side_reads() && !L.side_read(a0) && !L.find_act(a0) && !L.find_buf(a0));
    int n = 0;
    L.each_owed(OWED_GATE, [&](const void*, ActRec&) { ++n; });
    CHECK(n == 0);
    CHECK(!L.act(a0).has_g && L.act(a0).owed == 0);  // a fresh record
  }
  if (failures) {
    fprintf(stderr, "grad_ledger_check: %d failed\n", failures);
    return 1;
  }
  printf("grad_ledger_check: ok\n");
  return 0;
}
