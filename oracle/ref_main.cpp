// Entry point of oracle/_ref/abismal_ref: the reference's own `map` and `idx` commands, compiled from the reference's
// sources where they lie with the stand-in headers of ref_shims/ (see the Makefile's `ref` target).  Each command gets
// argv from its own name on, as the reference's main hands it over, so the SAM's @PG line reads as the reference's would.
#include <cstring>
#include <iostream>

#include "abismal.hpp"
#include "abismalidx.hpp"

int main(int argc, char *argv[]) {
  if (argc >= 2 && std::strcmp(argv[1], "map") == 0) return abismal(argc - 1, argv + 1);
  if (argc >= 2 && std::strcmp(argv[1], "idx") == 0) return abismalidx(argc - 1, argv + 1);
  std::cerr << "usage: abismal_ref {map|idx} ...\n";
  return 2;
}
