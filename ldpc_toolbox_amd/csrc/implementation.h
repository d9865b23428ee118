// Decoder implementation names <-> (check-node rule, precision, schedule).
//
// Mirrors the name table of the reference's decoder::factory::DecoderImplementation
// (/root/reference/src/decoder/factory.rs:240-277; FromStr error text :221) and adds the
// Minsum family this build defines.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace ldpc {

enum class Rule { Phi, Tanh, Minstarapprox, Aminstar, Minsum };
enum class Schedule { Flooding, Layered };
// Min-sum's magnitude correction ("NormMinsum" / "OffsetMinsum"; the values are those of the "minsum_correction" key)
enum class Correction { None = 0, Normalized = 1, Offset = 2 };

struct Implementation {
  Rule rule = Rule::Minsum;
  bool f64 = false;
  // 8-bit quantised arithmetics (rule is Minstarapprox, Aminstar or Minsum) and their options
  // (arithmetic.rs:806-848): Jones clipping, partial hard limiting, degree-one clipping
  bool i8 = false, jones = false, hardlimit = false, deg1clip = false;
  Schedule schedule = Schedule::Flooding;
  // "@fast" (Tanhf32 / Phif32, both schedules; this build's addition, never the default): the rule's formulas with the
  // GPU's native exp2 / log2 / rcp instead of the glibc-identical functions -- NOT bit-identical to the reference
  bool fast = false;
  // Normalized / offset min-sum (rule is Minsum, f32 / f64, both schedules; this build's addition): the magnitude m a plain
  // min-sum check row sends becomes  alpha * m  (Normalized, 0 < alpha <= 1)  or  max(m - beta, 0)  (Offset, beta >= 0),
  // with the message's sign as before.  correction_value is alpha or beta as given in the name (decimal, parsed to double;
  // converted once to the decoder's type where the kernels are launched).  The rule stays Rule::Minsum: everything the
  // decoder decides from the rule (L-free tables, row records, lanes, streaming, the small-batch paths) holds for these names.
  Correction correction = Correction::None;
  double correction_value = 0.0;
  // 8-bit min-sum (rule is Minsum, i8; this build's addition): "Minsumi8[Norm|Offset]<options>[:value]".  The magnitude m
  // (quantiser units, 0..127) becomes (a * m + 8) >> 4 with a = 16 alpha in 1..16 (Norm) or max(m - b, 0) with b = 8 beta in
  // 0..127 (Offset); correction_int is a or b (0 for the plain rule), correction_value the decimal as named.
  int correction_int = 0;
  // the one form the kernels evaluate: max(alpha * m - beta, 0)
  double alpha() const { return correction == Correction::Normalized ? correction_value : 1.0; }
  double beta() const { return correction == Correction::Offset ? correction_value : 0.0; }
  std::string name;
};

// Returns false and sets *err ("invalid decoder implementation" for unknown names,
// factory.rs:221).  All 36 names of the reference are accepted, plus the Minsum family and its corrected forms
// [HL]NormMinsum{f32,f64}[:alpha] (default 0.75) and [HL]OffsetMinsum{f32,f64}[:beta] (default 0.5); the value is
// digits[.digits] -- no sign, no exponent -- with 0 < alpha <= 1, beta >= 0 finite; and the 8-bit min-sum family
// [HL]Minsumi8[Norm|Offset][Jones][PartialHardLimit][Deg1Clip][:value] (HL: PartialHardLimit only; a value only after Norm or
// Offset, 16 alpha an integer in 1..16, default 0.75; 8 beta an integer in 0..127, default 0.5).
bool parse_implementation(const std::string &name, Implementation *out, std::string *err);

// "1,1,1,0" -> {1,1,1,0}; "" -> empty (no puncturing).  Only "0"/"1" tokens are legal
// (src/cli/ber.rs:219-229); returns false otherwise.
bool parse_puncturing_pattern(const std::string &text, std::vector<uint8_t> *out);

// Every name the HIP path accepts with results identical to the reference decoder's.
std::vector<std::string> implementation_names();
// The opt-in approximate variants ("Tanhf32@fast", "HLTanhf32@fast", "Phif32@fast", "HLPhif32@fast").
std::vector<std::string> fast_implementation_names();
// The normalized / offset min-sum names with their default values: [HL]{Norm,Offset}Minsum{f64,f32}, 8 names.
std::vector<std::string> corrected_minsum_implementation_names();
// The 8-bit min-sum names with their default values: 3 stems (Minsumi8, Minsumi8Norm, Minsumi8Offset) x (8 flooding option
// forms + HL with and without PartialHardLimit), 30 names.
std::vector<std::string> minsum_i8_implementation_names();

}  // namespace ldpc
