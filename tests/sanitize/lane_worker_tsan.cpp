// ThreadSanitizer harness for csrc/lane_worker.hpp and the hand-over protocols built on it (tests/test_sanitizers.py):
//   1. several producer threads post to several workers while other threads drain them;
//   2. the step queue's ticket protocol (environment.hpp, StepTicket): the worker writes `done`, then state (release); the
//      planner reads state (acquire), then `done`;
//   3. the batch calls' hand-over (post_with_result / wait_for_all, as segmentation.cpp's process_batch and
//      for_each_replica use them): the task shares the promise with the caller, every task is waited for although one throws,
//      and the first exception is the one the caller sees.
#include "lane_worker.hpp"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <future>
#include <memory>
#include <vector>

using dlimg::LaneWorker;

struct Ticket { std::atomic<int> state{0}; void* done = nullptr; };

int main() {
    long total = 0;
    {   // 1
        std::vector<std::unique_ptr<LaneWorker>> workers;
        for (int i = 0; i < 4; ++i) workers.push_back(std::make_unique<LaneWorker>());
        std::vector<long> sums(4, 0);                       // sums[w] is only touched by worker w's thread
        std::vector<std::thread> producers;
        for (int p = 0; p < 3; ++p)
            producers.emplace_back([&, p] {
                for (int i = 0; i < 2000; ++i) {
                    const int w = (i + p) % 4;
                    workers[w]->post([&sums, w, i] { sums[w] += i; });
                    if (i % 257 == 0) workers[(w + 1) % 4]->drain();
                }
            });
        for (auto& t : producers) t.join();
        for (auto& w : workers) w->drain();
        for (long s : sums) total += s;
        if (total != 3L * (1999L * 2000L / 2)) { std::printf("lost tasks: %ld\n", total); return 1; }
    }
    {   // 2
        LaneWorker worker;
        static int payload[64];
        std::vector<std::shared_ptr<Ticket>> tickets;
        for (int i = 0; i < 64; ++i) {
            auto t = std::make_shared<Ticket>();
            tickets.push_back(t);
            worker.post([t, i] {
                payload[i] = i * 7;
                t->done = &payload[i];
                t->state.store(1, std::memory_order_release);
            });
        }
        size_t retired = 0;
        while (retired < tickets.size()) {                  // the planner polls the oldest ticket, as retire_device_steps does
            Ticket& t = *tickets[retired];
            if (t.state.load(std::memory_order_acquire) == 0) { std::this_thread::yield(); continue; }
            if (*static_cast<int*>(t.done) != (int)retired * 7) { std::printf("ticket %zu: wrong payload\n", retired); return 1; }
            t.done = nullptr;
            ++retired;
        }
    }
    {   // 3
        LaneWorker a, b;
        for (int round = 0; round < 200; ++round) {
            int frame_local = round;                        // the tasks refer to the caller's frame, as run_chunk does
            const int thrower = round % 5 - 1;              // -1: nobody throws
            std::vector<std::future<int>> answers;
            for (int i = 0; i < 4; ++i)
                answers.push_back(dlimg::post_with_result(i & 1 ? a : b, [&frame_local, i, thrower] {
                    if (i == thrower || i == 3 - thrower) throw frame_local * 4 + i;
                    return frame_local * 4 + i;
                }));
            int got = 0, failed = 0, thrown = -1;
            try {
                dlimg::wait_for_all(
                    answers, nullptr, [&](size_t i, int v) { got += v == round * 4 + (int)i; }, [&](size_t) { ++failed; });
            } catch (int v) {
                thrown = v;
            }
            const int throwers = thrower < 0 ? 0 : 2;       // tasks `thrower` and 3 - thrower (never the same one)
            if (got != 4 - throwers || failed != throwers || thrown != (thrower < 0 ? -1 : round * 4 + std::min(thrower, 3 - thrower))) {
                std::printf("round %d: %d answers, %d failures, %d thrown\n", round, got, failed, thrown);
                return 1;
            }
            // void tasks beside the caller's own exception, which wins (for_each_replica)
            std::vector<std::future<void>> done;
            std::atomic<int> ran{0};
            for (int i = 0; i < 4; ++i)
                done.push_back(dlimg::post_with_result(i & 1 ? a : b, [&ran, i] { ++ran; if (i == 2) throw 2; }));
            try {
                dlimg::wait_for_all(done, std::make_exception_ptr(-7), [](size_t) {}, [](size_t) {});
                std::printf("round %d: no exception\n", round);
                return 1;
            } catch (int v) {
                if (v != -7 || ran != 4) { std::printf("round %d: thrown %d after %d tasks\n", round, v, (int)ran); return 1; }
            }
        }
    }
    std::printf("ok\n");
    return 0;
}
