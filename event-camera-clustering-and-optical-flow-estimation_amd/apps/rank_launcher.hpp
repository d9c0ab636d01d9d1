// One process per rank, forked before anything touches a GPU, with a blob created by rank 0 (the
// RCCL unique id of ecc_sharded_step) handed to the other ranks through pipes.  Needs nothing
// but POSIX, so a CPU program can drive it with ranks that never open a device
// (tests/rank_launcher_probe.cpp).  No exec anywhere: a rank is a fork of the launcher.
//
// A failed rank must not leave the others waiting:
//   * a pipe is open only where it is used: the parent closes every end once the ranks are
//     forked, rank 0 keeps the write ends, rank r > 0 its own read end.  If rank 0 dies before it
//     has written, no write end is left anywhere and the readers get EOF (and exit 1);
//   * the parent reaps in whatever order the ranks end; at the first one that exits non-zero or
//     by a signal it sends SIGTERM to those still running (they may sit in a collective that
//     cannot complete), reaps them too and returns non-zero.
#pragma once
#include <signal.h>
#include <sys/types.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <vector>

// make_blob(uint8_t *blob) -> bool   runs in rank 0's process and fills blob[blob_bytes]
// run_rank(int rank, int n_ranks, const uint8_t *blob) -> int   the rank's exit status
// Returns 0 when every rank exited 0, else 1.
template <class MakeBlob, class RunRank>
int launch_ranks(int n_ranks, size_t blob_bytes, MakeBlob make_blob, RunRank run_rank) {
    // one pipe per rank > 0: [2r] its read end, [2r + 1] the write end rank 0 uses
    std::vector<int> pipes(2 * (size_t)n_ranks, -1);
    auto close_unless = [&pipes](auto keep) {
        for (int i = 0; i < (int)pipes.size(); ++i)
            if (pipes[i] >= 0 && !keep(i)) {
                close(pipes[i]);
                pipes[i] = -1;
            }
    };
    const auto none = [](int) { return false; };
    for (int r = 1; r < n_ranks; ++r)
        if (pipe(&pipes[2 * r]) != 0) {
            std::perror("pipe");
            close_unless(none);
            return 1;
        }
    std::vector<pid_t> kids;
    bool failed = false;
    for (int r = 0; r < n_ranks; ++r) {
        const pid_t pid = fork();
        if (pid < 0) {
            std::perror("fork");
            failed = true;
            break;
        }
        if (pid == 0) {
            std::vector<uint8_t> blob(blob_bytes);
            if (r == 0) {
                close_unless([](int i) { return i % 2 == 1; });  // the write ends
                if (!make_blob(blob.data())) _exit(1);
                for (int q = 1; q < n_ranks; ++q) {
                    if (write(pipes[2 * q + 1], blob.data(), blob_bytes) != (ssize_t)blob_bytes) _exit(1);
                    close(pipes[2 * q + 1]);
                }
            } else {
                close_unless([r](int i) { return i == 2 * r; });  // its own read end
                size_t got = 0;
                while (got < blob_bytes) {
                    const ssize_t k = read(pipes[2 * r], blob.data() + got, blob_bytes - got);
                    if (k <= 0) _exit(1);  // EOF: rank 0 is gone
                    got += (size_t)k;
                }
                close(pipes[2 * r]);
            }
            std::fflush(stdout);
            _exit(run_rank(r, n_ranks, blob.data()));
        }
        kids.push_back(pid);
    }
    close_unless(none);
    auto terminate_rest = [&kids]() {
        for (pid_t k : kids)
            if (k > 0) kill(k, SIGTERM);
    };
    if (failed) terminate_rest();
    size_t left = kids.size();
    while (left > 0) {
        int st = 0;
        const pid_t done = waitpid(-1, &st, 0);
        if (done < 0 && errno == EINTR) continue;
        if (done < 0) break;  // ECHILD: nothing left to wait for
        bool ours = false;
        for (pid_t &k : kids)
            if (k == done) {
                k = -1;
                ours = true;
            }
        if (!ours) continue;
        --left;
        if ((!WIFEXITED(st) || WEXITSTATUS(st) != 0) && !failed) {
            failed = true;
            terminate_rest();
        }
    }
    return failed ? 1 : 0;
}
