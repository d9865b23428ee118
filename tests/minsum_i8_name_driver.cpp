// The implementation-name parser (csrc/implementation.cpp) under AddressSanitizer + UBSan, over the names given on the command
// line:  "+name=K,V" must parse, to the 8-bit min-sum rule with correction K (0 / 1 / 2) and integer V;  "-name" must be refused
// with "invalid decoder implementation".  Also: the name lists keep their sizes, and every listed name parses to itself.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../ldpc_toolbox_amd/csrc/implementation.h"

using namespace ldpc;

int main(int argc, char **argv) {
  int bad = 0;
  auto fail = [&](const std::string &what) {
    std::fprintf(stderr, "%s\n", what.c_str());
    bad++;
  };
  for (int a = 1; a < argc; a++) {
    const std::string arg = argv[a];
    Implementation impl;
    std::string err;
    if (arg[0] == '-') {
      if (parse_implementation(arg.substr(1), &impl, &err)) fail("accepted: " + arg);
      if (err != "invalid decoder implementation") fail("error text: " + arg);
      continue;
    }
    const size_t eq = arg.rfind('='), comma = arg.rfind(',');
    if (arg[0] != '+' || eq == std::string::npos || comma == std::string::npos || comma < eq) return 2;
    const std::string name = arg.substr(1, eq - 1);
    const int kind = std::atoi(arg.substr(eq + 1, comma - eq - 1).c_str()), value = std::atoi(arg.substr(comma + 1).c_str());
    if (!parse_implementation(name, &impl, &err)) {
      fail("refused: " + name);
      continue;
    }
    const bool layered = name.compare(0, 2, "HL") == 0;
    if (impl.name != name || impl.rule != Rule::Minsum || !impl.i8 || impl.f64 || impl.fast ||
        static_cast<int>(impl.correction) != kind || impl.correction_int != value ||
        (impl.schedule == Schedule::Layered) != layered || impl.jones != (name.find("Jones") != std::string::npos) ||
        impl.hardlimit != (name.find("PartialHardLimit") != std::string::npos) ||
        impl.deg1clip != (name.find("Deg1Clip") != std::string::npos))
      fail("parsed to something else: " + name);
  }
  if (implementation_names().size() != 40 || corrected_minsum_implementation_names().size() != 8 ||
      fast_implementation_names().size() != 4 || minsum_i8_implementation_names().size() != 30)
    fail("a name list changed its size");
  for (const auto &list : {implementation_names(), corrected_minsum_implementation_names(), fast_implementation_names(),
                           minsum_i8_implementation_names()})
    for (const std::string &name : list) {
      Implementation impl;
      std::string err;
      if (!parse_implementation(name, &impl, &err) || impl.name != name) fail("listed but refused: " + name);
    }
  for (const std::string &name : implementation_names()) {
    Implementation impl;
    std::string err;
    if (parse_implementation(name, &impl, &err) && impl.correction_int != 0) fail("correction_int set: " + name);
  }
  if (bad) return 1;
  std::printf("minsum i8 name driver: ok (%d names)\n", argc - 1);
  return 0;
}
