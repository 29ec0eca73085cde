// muchsalsa_gpu -- the reference's executable on libmsgpu, no Python in the process:
//     muchsalsa_gpu <contigs.paf> <unitigs.fa> <nanopore.fa|fq> <outdir> [threads] [wiggleRoom = 300]
// (the argument list of src/Application.cpp:34-39; writes outdir/temp_1.target.fa, temp_1.query.fa, temp_1.align.paf like
// src/main.cpp:130-322).  The body of main() is msgpu::assemble (include/msgpu_adapter.hpp): straight calls into the C-ABI.
#include <cctype>
#include <cerrno>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <string>
#include <thread>

#include "msgpu_adapter.hpp"

// wiggleRoom as the reference reads it (src/Application.cpp:76): static_cast<size_t>(std::stoi(arg)), so "-1" is 2^64 - 1, no
// limit.  The whole argument must be an integer in int's range; anything else is refused (where stoi would throw).
static bool parse_wiggle(const char *s, std::size_t *out) {
  if (!(std::isdigit(static_cast<unsigned char>(s[0])) || s[0] == '-' || s[0] == '+')) return false;
  errno          = 0;
  char      *end = nullptr;
  const long v   = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || errno == ERANGE || v < INT_MIN || v > INT_MAX) return false;
  *out = static_cast<std::size_t>(static_cast<int>(v));
  return true;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s <contigs.paf> <unitigs.fa> <nanopore.fa|fq> <outdir> [threads] [wiggleRoom=300]\n", argv[0]);
    return -1; // Application::checkIntegrity failing (src/main.cpp:134-137)
  }
  unsigned threads = std::thread::hardware_concurrency();
  threads          = threads == 0 ? 1 : (threads > 16 ? 16 : threads);
  if (argc > 5) threads = static_cast<unsigned>(std::max(1, std::atoi(argv[5])));
  std::size_t wiggle = 300;
  if (argc > 6 && !parse_wiggle(argv[6], &wiggle)) {
    std::fprintf(stderr, "muchsalsa_gpu: wiggleRoom must be an integer, got '%s'\n", argv[6]);
    return 2;
  }
  try {
    const msgpu::AssemblyCounts n = msgpu::assemble(argv[1], argv[2], argv[3], argv[4], threads, wiggle, 0);
    std::printf("{\"rows\": %llu, \"reads\": %llu, \"edges\": %llu, \"orders\": %llu, \"contraction_edges\": %llu, \"paths\": %llu, "
                "\"paths_skipped\": %llu, \"contigs\": %llu, \"target_bases\": %llu, \"queries\": %llu}\n",
                static_cast<unsigned long long>(n.rows), static_cast<unsigned long long>(n.reads),
                static_cast<unsigned long long>(n.edges), static_cast<unsigned long long>(n.orders),
                static_cast<unsigned long long>(n.contractionEdges), static_cast<unsigned long long>(n.paths),
                static_cast<unsigned long long>(n.pathsSkipped), static_cast<unsigned long long>(n.contigs),
                static_cast<unsigned long long>(n.targetBases), static_cast<unsigned long long>(n.queries));
    std::puts("Finished assembly"); // src/main.cpp:320
  } catch (std::exception const &e) {
    std::fprintf(stderr, "muchsalsa_gpu: %s\n", e.what());
    return 1;
  }
  return 0;
}
