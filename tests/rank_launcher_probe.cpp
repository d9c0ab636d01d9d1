// CPU probe of apps/rank_launcher.hpp (tests/test_rank_launcher.py compiles and runs it): four
// ranks that never touch a GPU, in one of three scenarios.
//   rank0_dies_early   rank 0 exits 1 before it has sent the blob; the other ranks would sleep 60 s
//   rank2_fails_late   rank 2 exits 1 once it has the blob; the other ranks sleep 60 s
//   all_ok             every rank prints the blob it received and exits 0
// Exit status: the launcher's.
#include <unistd.h>

#include <cstring>
#include <string>

#include "rank_launcher.hpp"

namespace {
constexpr size_t kBlob = 128;

int print_blob(int rank, const uint8_t *blob) {
    std::string line = "rank " + std::to_string(rank) + " ";
    for (size_t i = 0; i < kBlob; ++i) {
        static const char hex[] = "0123456789abcdef";
        line += hex[blob[i] >> 4];
        line += hex[blob[i] & 15];
    }
    line += "\n";
    return write(1, line.data(), line.size()) == (ssize_t)line.size() ? 0 : 1;  // one write: lines do not mix
}
}  // namespace

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode != "rank0_dies_early" && mode != "rank2_fails_late" && mode != "all_ok") return 2;
    const bool early = mode == "rank0_dies_early", late = mode == "rank2_fails_late";
    return launch_ranks(
        4, kBlob,
        [early](uint8_t *blob) {
            if (early) _exit(1);
            for (size_t i = 0; i < kBlob; ++i) blob[i] = (uint8_t)(i * 7 + 3);
            return true;
        },
        [early, late](int rank, int, const uint8_t *blob) {
            if (late && rank == 2) return 1;
            if (early || late) {
                sleep(60);
                return 0;
            }
            return print_blob(rank, blob);
        });
}
