// The host half of iupac_marks_check on its own (no device): prints the counts the fixtures must give, so that they can be
// checked where there is no GPU.  Built and run by tests/test_gpu_iupac_marks.py::test_host_half_counts.
#include "iupac_marks_host.hpp"

int main() {
  const marks::Counts c = marks::expected_counts();
  std::printf("OK host ");
  marks::print_counts(c);
  return c.must_on > c.must_off && c.rec_on > c.rec_off && c.rec_off > 0 && c.rec_on < c.rec && c.last_covered > 0 && c.first_past > 0 && c.under_padding > 0 && c.past_padding > 0 ? 0 : 1;
}
