// tests/native/zero_ledger_check.cpp -- giql_amd/csrc/zero_ledger.h without a GPU: the ledger of the workspace bytes
// that were zeroed up front (what it covers, what it hands over once and refuses afterwards, how its range grows) and
// the Carver's zeroed span.  The addresses are offsets into one host array that is never written.  Stand-alone: builds
// with any C++17 compiler, with or without -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>

#include "../../giql_amd/csrc/zero_ledger.h"

using namespace giql;

static int g_failed = 0;

static void report(const char* name, bool ok) {
  printf("%s zero_ledger: %s\n", ok ? "ok  " : "FAIL", name);
  if (!ok) g_failed++;
}

struct Layout {
  uint32_t *before, *hist, *status, *after;
  uint64_t* wide;
  ZeroSpan zero;
  size_t size;
};

// a carve with a zeroed span in its middle, entered at an odd offset and left at one
static Layout carve(char* base) {
  Layout l;
  Carver c{base};
  l.before = c.take<uint32_t>(3);
  c.take<char>(1);
  c.open_zeroed();
  l.hist = c.take<uint32_t>(1000);
  l.wide = c.take<uint64_t>(5);
  l.status = c.take<uint32_t>(77);
  l.zero = c.close_zeroed();
  l.after = c.take<uint32_t>(9);
  l.size = c.off;
  return l;
}

int main() {
  alignas(256) static char mem[8192];
  char* const lo = mem + 1024;  // the zeroed range of most cases: [lo, lo + 2048)
  {
    ZeroLedger z;
    report("an empty ledger covers nothing",
           !z.covers(lo, 16) && !z.covers(nullptr, 16) && !z.take(lo, 16) && !z.covers(lo, 0) && z.end() == nullptr);
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    const bool first = z.covers(lo + 256, 512) && z.take(lo + 256, 512);
    const bool again = !z.covers(lo + 256, 512) && !z.take(lo + 256, 512);
    // (what touches a taken buffer anywhere is refused as well; its neighbours are not)
    const bool overlap = !z.take(lo + 512, 16) && !z.take(lo, 257) && !z.take(lo, 2048);
    const bool beside = z.take(lo, 256) && z.take(lo + 768, 1280);
    report("a buffer inside the range is taken once and refused the second time", first && again && overlap && beside);
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    const bool refused = !z.covers(lo - 4, 8) && !z.take(lo - 4, 8) && !z.covers(lo + 2044, 8) && !z.take(lo + 2044, 8) &&
                         !z.take(lo - 4, 4096);
    report("a buffer that straddles either end is refused", refused && z.take(lo, 2048));  // (the whole range is inside)
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    report("a buffer outside is refused", !z.take(mem, 1024) && !z.take(lo - 256, 256) && !z.take(lo + 2048, 4) &&
                                              !z.take(lo + 4096, 4) && !z.take(lo, SIZE_MAX));
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    const bool before = !z.covers(lo + 2000, 100) && z.end() == lo + 2048;
    z.add(lo + 2048, 512);
    report("add at the end of the range extends it",
           before && z.end() == lo + 2560 && z.covers(lo + 2000, 100) && z.take(lo + 2000, 560) && !z.take(lo + 2560, 4));
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    z.take(lo, 64);
    z.add(lo + 2304, 256);  // past the end, a gap between
    z.add(lo - 256, 256);   // ends where the range begins
    z.add(lo + 512, 4096);  // overlaps the end
    z.add(mem, 64);
    z.add(lo + 2048, 0);
    z.add(nullptr, 64);
    report("add anywhere else leaves the ledger as it was",
           z.end() == lo + 2048 && !z.covers(lo + 2304, 16) && !z.covers(lo - 256, 16) && !z.covers(mem, 16) &&
               !z.covers(lo + 2040, 16) && !z.covers(lo, 64) && z.covers(lo + 64, 1984));
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    bool ok = true;
    for (int i = 0; i < ZeroLedger::MAX_TAKEN; i++) ok = ok && z.take(lo + 64 * i, 64);
    char* const next = lo + 64 * ZeroLedger::MAX_TAKEN;
    ok = ok && z.covers(next, 64) && !z.take(next, 64) && !z.take(next, 64) && z.covers(next, 64);
    report("the taken list, once full, refuses", ok && ZeroLedger::MAX_TAKEN >= 10);
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    z.take(lo, 64);
    z.reset();
    const bool forgot = z.end() == nullptr && !z.covers(lo + 64, 64) && !z.take(lo, 64);
    z.add(lo + 4096, 128);  // (a range of its own afterwards, and the buffer taken before is free again)
    z.add(lo + 4224, 128);
    z.reset();
    z.add(lo, 2048);
    report("reset forgets the range and the taken list", forgot && z.take(lo, 64) && z.end() == lo + 2048);
  }
  {
    ZeroLedger z;
    z.add(lo, 2048);
    bool ok = z.covers(lo, 0) && z.covers(lo + 2048, 0) && !z.covers(lo - 1, 0) && !z.covers(lo + 2049, 0);
    // nothing to zero: handed over as often as asked, no entry used, and the buffer at that address stays free
    for (int i = 0; i < 2 * ZeroLedger::MAX_TAKEN; i++) ok = ok && z.take(lo + 128, 0);
    ok = ok && z.take(lo + 128, 64) && z.take(lo + 128, 0) && !z.take(lo + 160, 0) && z.take(lo + 192, 0);
    report("a zero-byte buffer", ok);
  }
  {
    const Layout dry = carve(nullptr);
    const Layout real = carve(mem);
    const bool aligned = dry.zero.off % 256 == 0 && dry.zero.end % 256 == 0 && dry.zero.off == 512 &&
                         dry.zero.end == 512 + 4096 + 256 + 512;  // (4000 + 40 + 308 bytes, each buffer 256-aligned)
    const bool same = dry.zero.off == real.zero.off && dry.zero.end == real.zero.end && dry.size == real.size &&
                      !dry.hist && !dry.status && !dry.after;
    const bool inside = (char*)real.hist == mem + real.zero.off && (char*)(real.status + 77) <= mem + real.zero.end &&
                        (char*)(real.before + 3) <= mem + real.zero.off && (char*)real.after == mem + real.zero.end;
    // the span as the ledger's range: every buffer carved inside it is covered, its neighbours are not
    ZeroLedger z;
    z.add(mem + real.zero.off, real.zero.end - real.zero.off);
    const bool led = z.take(real.hist, 4000) && z.take(real.wide, 40) && z.take(real.status, 308) &&
                     !z.take(real.before, 12) && !z.take(real.after, 36);
    report("the Carver's zeroed span is 256-aligned at both ends, a dry run gives the same offsets",
           aligned && same && inside && led);
  }
  if (g_failed) {
    printf("%d case(s) failed\n", g_failed);
    return 1;
  }
  printf("all cases passed\n");
  return 0;
}
