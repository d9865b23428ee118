#include "implementation.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

namespace ldpc {

namespace {
struct Stem {
  const char *text;
  Rule rule;
};
const Stem kStems[] = {{"Phi", Rule::Phi},
                       {"Tanh", Rule::Tanh},
                       {"Minstarapprox", Rule::Minstarapprox},
                       {"Aminstar", Rule::Aminstar},
                       {"Minsum", Rule::Minsum}};
struct CorrectedStem {
  const char *text;
  Correction correction;
  double dflt;
};
const CorrectedStem kCorrectedStems[] = {{"NormMinsum", Correction::Normalized, 0.75}, {"OffsetMinsum", Correction::Offset, 0.5}};

// digits[.digits], nothing else (no sign, no exponent, no "inf"): what strtod is then allowed to see
bool plain_decimal(const char *p) {
  const char *q = p;
  while (*q >= '0' && *q <= '9') q++;
  if (q == p) return false;
  if (*q == '.') {
    const char *f = ++q;
    while (*q >= '0' && *q <= '9') q++;
    if (q == f) return false;
  }
  return *q == 0;
}
}  // namespace

bool parse_implementation(const std::string &name, Implementation *out, std::string *err) {
  Implementation impl;
  impl.name = name;
  const char *p = name.c_str();
  if (std::strncmp(p, "HL", 2) == 0) {
    impl.schedule = Schedule::Layered;
    p += 2;
  }
  for (const CorrectedStem &s : kCorrectedStems) {
    const size_t l = std::strlen(s.text);
    if (std::strncmp(p, s.text, l) != 0) continue;
    const char *suffix = p + l;
    if (std::strncmp(suffix, "f32", 3) != 0 && std::strncmp(suffix, "f64", 3) != 0) break;  // (the 8-bit forms are spelled Minsumi8Norm / Minsumi8Offset)
    Implementation c = impl;
    c.rule = Rule::Minsum;
    c.f64 = suffix[1] == '6';
    c.correction = s.correction;
    c.correction_value = s.dflt;
    suffix += 3;
    if (*suffix == ':') {
      if (!plain_decimal(suffix + 1)) break;
      c.correction_value = std::strtod(suffix + 1, nullptr);
    } else if (*suffix != 0) {
      break;  // ("@fast" included: there is no approximate form of these)
    }
    const double v = c.correction_value;
    if (!std::isfinite(v) || (s.correction == Correction::Normalized ? !(v > 0.0 && v <= 1.0) : !(v >= 0.0))) break;
    *out = c;
    return true;
  }
  for (const Stem &s : kStems) {
    const size_t l = std::strlen(s.text);
    if (std::strncmp(p, s.text, l) != 0) continue;
    const char *suffix = p + l;
    if (std::strcmp(suffix, "f32") == 0 || std::strcmp(suffix, "f64") == 0) {
      impl.rule = s.rule;
      impl.f64 = suffix[1] == '6';
      *out = impl;
      return true;
    }
    if (std::strcmp(suffix, "f32@fast") == 0 && (s.rule == Rule::Tanh || s.rule == Rule::Phi)) {
      impl.rule = s.rule;
      impl.fast = true;
      *out = impl;
      return true;
    }
    if (std::strncmp(suffix, "i8", 2) == 0 && s.rule != Rule::Phi && s.rule != Rule::Tanh) {
      // factory.rs:246-263, 270-275: optional Jones / PartialHardLimit / Deg1Clip, in this order;
      // the layered schedule exists only with and without PartialHardLimit
      const char *q = suffix + 2;
      impl.rule = s.rule;
      impl.i8 = true;
      if (s.rule == Rule::Minsum) {
        // Minsumi8[Norm|Offset]<options>[:value]: the correction follows "i8", its value the options
        if (std::strncmp(q, "Norm", 4) == 0) {
          impl.correction = Correction::Normalized;
          impl.correction_value = 0.75;
          q += 4;
        } else if (std::strncmp(q, "Offset", 6) == 0) {
          impl.correction = Correction::Offset;
          impl.correction_value = 0.5;
          q += 6;
        }
      }
      if (std::strncmp(q, "Jones", 5) == 0) {
        impl.jones = true;
        q += 5;
      }
      if (std::strncmp(q, "PartialHardLimit", 16) == 0) {
        impl.hardlimit = true;
        q += 16;
      }
      if (std::strncmp(q, "Deg1Clip", 8) == 0) {
        impl.deg1clip = true;
        q += 8;
      }
      if (*q == ':' && impl.correction != Correction::None && plain_decimal(q + 1)) {
        impl.correction_value = std::strtod(q + 1, nullptr);
        q += std::strlen(q);
      }
      if (impl.correction != Correction::None) {
        // the kernels' integers: a = 16 alpha in 1..16, b = 8 beta in 0..127, exactly
        const bool norm = impl.correction == Correction::Normalized;
        const double scaled = impl.correction_value * (norm ? 16.0 : 8.0);
        if (!(scaled >= (norm ? 1.0 : 0.0) && scaled <= (norm ? 16.0 : 127.0)) || scaled != std::floor(scaled)) break;
        impl.correction_int = static_cast<int>(scaled);
      }
      if (*q == 0 && !(impl.schedule == Schedule::Layered && (impl.jones || impl.deg1clip))) {
        *out = impl;
        return true;
      }
    }
  }
  if (err) *err = "invalid decoder implementation";
  return false;
}

bool parse_puncturing_pattern(const std::string &text, std::vector<uint8_t> *out) {
  out->clear();
  if (text.empty()) return true;
  size_t start = 0;
  while (true) {
    const size_t comma = text.find(',', start);
    const std::string tok = text.substr(start, comma == std::string::npos ? std::string::npos : comma - start);
    if (tok != "0" && tok != "1") return false;
    out->push_back(tok == "1");
    if (comma == std::string::npos) break;
    start = comma + 1;
  }
  return true;
}

std::vector<std::string> fast_implementation_names() {
  return {"Tanhf32@fast", "HLTanhf32@fast", "Phif32@fast", "HLPhif32@fast"};
}

std::vector<std::string> corrected_minsum_implementation_names() {
  std::vector<std::string> v;
  for (const char *prefix : {"", "HL"})
    for (const CorrectedStem &s : kCorrectedStems)
      for (const char *suffix : {"f64", "f32"}) v.push_back(std::string(prefix) + s.text + suffix);
  return v;
}

std::vector<std::string> minsum_i8_implementation_names() {
  std::vector<std::string> v;
  for (const char *base : {"Minsumi8", "Minsumi8Norm", "Minsumi8Offset"}) {
    for (const char *j : {"", "Jones"})
      for (const char *h : {"", "PartialHardLimit"})
        for (const char *d : {"", "Deg1Clip"}) v.push_back(std::string(base) + j + h + d);
    v.push_back(std::string("HL") + base);
    v.push_back(std::string("HL") + base + "PartialHardLimit");
  }
  return v;
}

std::vector<std::string> implementation_names() {
  std::vector<std::string> v;
  for (const char *prefix : {"", "HL"})
    for (const Stem &s : kStems)
      for (const char *suffix : {"f64", "f32"}) v.push_back(std::string(prefix) + s.text + suffix);
  for (const char *base : {"Minstarapproxi8", "Aminstari8"}) {
    for (const char *j : {"", "Jones"})
      for (const char *h : {"", "PartialHardLimit"})
        for (const char *d : {"", "Deg1Clip"}) v.push_back(std::string(base) + j + h + d);
    v.push_back(std::string("HL") + base);
    v.push_back(std::string("HL") + base + "PartialHardLimit");
  }
  return v;
}

}  // namespace ldpc
