// Host-side walk of the option table (loraine.jl_amd/csrc/options.h): every key of kOptions with every probe value of
// tests/option_cases.py that its conversion is defined for, through option_apply on a plain LrnOptions.  Checks what holds for any
// table -- a reject stores nothing and carries a text, a clamp ends inside its range, a key is found under its own name only --
// and is the program to run under -fsanitize=address,undefined (no context, no device).  Built by tests/test_options_cpu.py with
// hipcc (host code only, no GPU needed).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "ctx.h"
#include "options.h"
using namespace lrn;

int main() {
  const double values[] = {-2, -1, 0, 0.5, 1, 2, 3, 17, 127, 200, 1e6, 1e10, std::nan("")};
  int bad = 0, stored = 0, rejected = 0;
  for (const OptionDesc& t : kOptions) {
    const bool guarded = t.rule == OPT_REJECT || t.rule == OPT_ZERO_OR_ONE;      // the value is tested before any cast
    for (double v : values) {
      // (int)v of a value that does not fit, or of NaN, is undefined in the chain this table replaced as well: not walked
      if (!guarded && (t.i || t.l) && t.rule != OPT_NONZERO && (std::isnan(v) || (t.i && std::fabs(v) > 2.0e9))) continue;
      LrnOptions o, before;
      unsigned fx = ~0u;
      const char* msg = nullptr;
      const int rc = option_apply(o, t.name, v, &fx, &msg);
      if (rc == OPT_ERR_ARG) {
        ++rejected;
        if (!guarded || !msg || !*msg || fx != ~0u) ++bad;
        if (t.i && o.*t.i != before.*t.i) ++bad;
        if (t.l && o.*t.l != before.*t.l) ++bad;
        if (t.d && o.*t.d != before.*t.d) ++bad;
        continue;
      }
      if (rc != OPT_OK || fx != t.effects || msg) { ++bad; continue; }
      ++stored;
      if (t.rule == OPT_CLAMP && t.i && (o.*t.i < t.lo || o.*t.i > t.hi)) ++bad;
      if (t.rule == OPT_NONZERO && t.i && o.*t.i != (v != 0.0)) ++bad;
      if (t.flag && o.*t.flag != (v != 0.0)) ++bad;
      if (t.rule == OPT_MASK && (o.*t.i & ~(int)t.hi)) ++bad;
    }
    int named = 0;
    for (const OptionDesc& u : kOptions) named += !strcmp(u.name, t.name);
    for (const char* k : kContextOptions) named += !strcmp(k, t.name);
    if (named != 1) ++bad;
    if (((t.i != nullptr) + (t.l != nullptr) + (t.d != nullptr) + (t.flag != nullptr)) != 1) ++bad;
  }
  LrnOptions o;
  unsigned fx = 0;
  const char* msg = nullptr;
  for (const char* k : kContextOptions)
    if (option_apply(o, k, 1.0, &fx, &msg) != OPT_NOT_A_VALUE) ++bad;
  if (option_apply(o, "no_such_option", 1.0, &fx, &msg) != OPT_NOT_A_VALUE || option_apply(o, "", 1.0, &fx, &msg) != OPT_NOT_A_VALUE) ++bad;
  for (int i = 0; i < kNumOptions + kNumContextOptions; ++i)
    if (!option_name(i)) ++bad;
  if (option_name(-1) || option_name(kNumOptions + kNumContextOptions)) ++bad;
  std::printf("options=%d context=%d stored=%d rejected=%d bad=%d\n", kNumOptions, kNumContextOptions, stored, rejected, bad);
  return bad != 0;
}
