// Stand-alone check of mgdt_yolo_amd/csrc/launch_host.h (built and run by tests/test_launch_host.py with the host compiler, sanitizers where they link).
// Every expectation is a number worked out by hand, not a second copy of the header's formulas.
#include <stdio.h>
#include <stdlib.h>

#include "../../mgdt_yolo_amd/csrc/launch_host.h"

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) { printf("FAIL line %d: %s\n", __LINE__, #cond); ++failures; } \
  } while (0)

static void* const BASE = (void*)0x1000;      // never dereferenced

// one pixel row of c channels
static mgdt_view row(int c) { return mgdt_view{BASE, 1, 1, 1, c, c, c, c, 1}; }

struct Out { const char* p; int sn, sh, sw; uint32_t bytes; };
static const Out UNTOUCHED = {(const char*)0x77, -1, -2, -3, 0xabcdu};
static bool bind(const mgdt_view* v, int elem, const ViewPolicy& pol, Out* o) {
  *o = UNTOUCHED;
  return bind_view(v, elem, pol, &o->p, &o->sn, &o->sh, &o->sw, &o->bytes);
}
static bool untouched(const Out& o) { return o.p == UNTOUCHED.p && o.sn == -1 && o.sh == -2 && o.sw == -3 && o.bytes == 0xabcdu; }

static const ViewPolicy PLAIN = {0, false, 0, 0, false};
static const ViewPolicy IGEMM = {0, false, 1L << 23, 1L << 23, true};       // conv_igemm.hip
static const ViewPolicy WGRAD_MFMA = {0, false, 1L << 28, 0, false};        // wgrad_mfma.hip

static void check_extent() {
  Out o;
  // 2-byte elements: 1073741823 of them end at byte 2^31 - 3 (extent 2147483646); one more reaches 2^31
  mgdt_view v = row(1073741823);
  CHECK(view_extent_bytes(&v, 2) == 2147483646L);
  CHECK(bind(&v, 2, PLAIN, &o) && o.bytes == 2147483646u);
  v = row(1073741824);
  CHECK(view_extent_bytes(&v, 2) == 2147483648L);
  CHECK(!bind(&v, 2, PLAIN, &o) && untouched(o));
  // 4-byte elements cannot end at 2^31 - 3: the longest view below the limit has 536870911 of them (extent 2147483644, last byte 2^31 - 5)
  v = row(536870911);
  CHECK(bind(&v, 4, PLAIN, &o) && o.bytes == 2147483644u);
  v = row(536870912);
  CHECK(!bind(&v, 4, PLAIN, &o) && untouched(o));
  // the extent counts the strides, not the sizes: two rows 2^30 - 8 elements apart, 2 bytes each, 7 channels -> (1073741816 + 7) * 2
  v = mgdt_view{BASE, 1, 2, 1, 7, 0, 1073741816, 7, 1};
  CHECK(bind(&v, 2, PLAIN, &o) && o.bytes == 2147483646u && o.sh == 2147483632);
  v.c = 8;
  CHECK(!bind(&v, 2, PLAIN, &o));
}

// n = 2, h = 3, w = 5, c = 8: a channel slice of a 24-channel buffer whose rows hold 7 pixels and whose images hold 5 rows
static mgdt_view sliced() { return mgdt_view{BASE, 2, 3, 5, 8, 840, 168, 24, 1}; }

static void check_outputs() {
  Out o;
  mgdt_view v = sliced();
  // elements: 1 * 840 + 2 * 168 + 4 * 24 + 8 = 1280
  CHECK(view_extent_bytes(&v, 2) == 2560 && view_extent_bytes(&v, 4) == 5120);
  CHECK(bind(&v, 2, {4, true, 0, 0, false}, &o));
  CHECK(o.p == (const char*)BASE && o.sn == 1680 && o.sh == 336 && o.sw == 48 && o.bytes == 2560u);
  CHECK(bind(&v, 4, {4, true, 1L << 23, 1L << 23, false}, &o));
  CHECK(o.sn == 3360 && o.sh == 672 && o.sw == 96 && o.bytes == 5120u);
  CHECK(view_fits(&v, 2, {8, true, 0, 0, false}) && view_spans_32bit(&v, 2));
}

static void check_alignment() {
  Out o;
  const ViewPolicy al4 = {4, true, 0, 0, false}, al0 = {0, true, 0, 0, false};
  mgdt_view v = sliced();
  CHECK(bind(&v, 2, al4, &o));
  v.p = (void*)0x1002;                                      // one 2-byte element off
  CHECK(!bind(&v, 2, al4, &o) && untouched(o));
  CHECK(bind(&v, 2, al0, &o) && o.p == (const char*)0x1002);
  v.p = (void*)0x1004;                                      // 4 elements of 2 bytes = 8-byte pieces: 4 bytes off is refused, 8 bytes is not
  CHECK(!bind(&v, 2, al4, &o));
  v.p = (void*)0x1008;
  CHECK(bind(&v, 2, al4, &o));
  v = sliced(); v.sh = 167;                                 // one short of 168 = 4 * 42
  CHECK(!bind(&v, 2, al4, &o) && untouched(o));
  CHECK(bind(&v, 2, al0, &o) && o.sh == 334);
  v = sliced(); v.sn = 839;
  CHECK(!bind(&v, 2, al4, &o));
  v = sliced(); v.sw = 23;
  CHECK(!bind(&v, 2, al4, &o));
  v = sliced();
  CHECK(view_aligned(&v, 8, 2) && !view_aligned(&v, 16, 2));   // 840 = 8 * 105, 168 = 8 * 21, 24 = 8 * 3
}

static void check_sc() {
  Out o;
  mgdt_view v = sliced();
  v.sc = 2;
  CHECK(!bind(&v, 2, {4, true, 0, 0, false}, &o) && untouched(o));
  CHECK(bind(&v, 2, {4, false, 0, 0, false}, &o) && o.bytes == 2560u);
}

static void check_stride_limits() {
  Out o;
  // two rows, 2-byte elements: a row stride of 4194304 elements is 2^23 bytes
  mgdt_view v = mgdt_view{BASE, 1, 2, 1, 8, 0, 4194304, 8, 1};
  CHECK(!bind(&v, 2, IGEMM, &o) && untouched(o));
  CHECK(bind(&v, 2, WGRAD_MFMA, &o) && o.sh == 8388608);
  v.sh = 4194303;                                           // 2^23 - 2 bytes
  CHECK(bind(&v, 2, IGEMM, &o) && o.sh == 8388606);
  // the pixel stride has its own limit under the igemm policy and none under the wgrad one
  v = mgdt_view{BASE, 1, 1, 2, 8, 0, 0, 4194304, 1};
  CHECK(!bind(&v, 2, IGEMM, &o));
  CHECK(bind(&v, 2, WGRAD_MFMA, &o) && o.sw == 8388608);
  v.sw = 4194303;
  CHECK(bind(&v, 2, IGEMM, &o) && o.sw == 8388606);
  // 134217728 elements of 2 bytes = 2^28 bytes
  v = mgdt_view{BASE, 1, 2, 1, 8, 0, 134217728, 8, 1};
  CHECK(!bind(&v, 2, WGRAD_MFMA, &o) && untouched(o));
  CHECK(bind(&v, 2, PLAIN, &o) && o.sh == 268435456);
  v.sh = 134217727;                                         // 2^28 - 2 bytes
  CHECK(bind(&v, 2, WGRAD_MFMA, &o) && o.sh == 268435454);
}

static void check_null() {
  Out o;
  mgdt_view v = sliced();
  v.p = nullptr;
  bool fits = true;
  fits &= bind(nullptr, 2, IGEMM, &o);
  CHECK(fits && untouched(o));
  fits &= bind(&v, 2, IGEMM, &o);
  CHECK(fits && untouched(o));
  CHECK(!bind(nullptr, 2, PLAIN, &o) && untouched(o));
  CHECK(!bind(&v, 2, PLAIN, &o) && untouched(o));
}

static int once_int() { return KNOB_ONCE(knob_int("MGDT_CHECK_KNOB", -1)); }

static void check_knobs() {
  const char* K = "MGDT_CHECK_KNOB";
  // value (NULL = unset), knob_int / knob_long with default 42, knob_set, knob_unless0, knob_pair scans
  struct Case { const char* val; int i; bool set, unless0, pair; };
  const Case cases[] = {
      {nullptr, 42, false, true, false}, {"", 0, true, true, false},   {"0", 0, true, false, false},
      {"1", 1, true, true, false},       {"07", 7, true, false, false}, {"x", 0, true, true, false},
      {"5,10", 5, true, true, true},     {"5,", 5, true, true, false},  {"5", 5, true, true, false},
  };
  for (const Case& c : cases) {
    if (c.val) setenv(K, c.val, 1); else unsetenv(K);
    int a = -7, b = -8;
    const bool scanned = knob_pair(K, &a, &b);
    const bool ok = knob_int(K, 42) == c.i && knob_long(K, 42) == (long)c.i && knob_set(K) == c.set && knob_unless0(K) == c.unless0 && scanned == c.pair &&
                    (c.pair ? a == 5 && b == 10 : a == -7 && b == -8);
    if (!ok) { printf("FAIL knob value %s\n", c.val ? c.val : "(unset)"); ++failures; }
  }
  setenv(K, "3", 1);
  CHECK(once_int() == 3);
  setenv(K, "9", 1);
  CHECK(once_int() == 3);             // cached for the life of the process
  CHECK(knob_int(K, -1) == 9);        // read per call
  unsetenv(K);
  CHECK(once_int() == 3 && knob_int(K, -1) == -1);
  unsetenv("MGDT_STEM_WGS");
  CHECK(knob_stem_wgs() == 0);
  setenv("MGDT_STEM_WGS", "2", 1);
  CHECK(knob_stem_wgs() == 2);
  unsetenv("MGDT_STEM_WGS");
}

int main() {
  check_extent();
  check_outputs();
  check_alignment();
  check_sc();
  check_stride_limits();
  check_null();
  check_knobs();
  printf(failures ? "launch_host_check: %d failures\n" : "launch_host_check: ok\n", failures);
  return failures ? 1 : 0;
}
