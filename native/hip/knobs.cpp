// The launch knobs' table and values (GS_KNOBS of api.h).  Host code only: the knobs are plain statics read
// on the launching host thread (gemm.hip tells why that is sound), and a table defined in a .hip file would
// be emitted into the device code as well.
#include <stdexcept>
#include <string>

#include "api.h"

namespace gs {

#define GS_KNOB_INFO(name, lo, hi, def, kind) {#name, lo, hi, def, kind},
const KnobInfo kKnobs[kNumKnobs] = {GS_KNOBS(GS_KNOB_INFO)};
#define GS_KNOB_DEFAULT(name, lo, hi, def, kind) def,
int g_knob[kNumKnobs] = {GS_KNOBS(GS_KNOB_DEFAULT)};

void reset_knobs() {
  for (int k = 0; k < kNumKnobs; ++k) g_knob[k] = kKnobs[k].def;
}

void set_knob(Knob k, int v) {
  const KnobInfo& i = kKnobs[k];
  if (i.kind == ON_OFF) v = v ? 1 : 0;
  else if (v < i.min || v > i.max)
    throw std::runtime_error(std::string(i.name) + " must be " + std::to_string(i.min) + ".." + std::to_string(i.max));
  g_knob[k] = k == k_split_k && v == 1 ? 0 : v;      // one K slice is no split
}

}  // namespace gs
