// Prints the plan csrc/mask_transport.hpp makes for one request, for tests/test_mask_transport.py to compare with what the
// rules say (built there with the host compiler: the planner needs no HIP and no GPU).
//   mask_transport_cases host <direct_allowed> <others_idle> <iou_count> [<bytes>:<dst pinned>]...
//   mask_transport_cases device <kernel_writes_dst> [<bytes>]...
// Output, one line each: mode, launches, kernel_dst (offsets, `caller`), in_place, piece_end, iou_offset, reserve (device,
// pinned), pieces_agree (piece_end == mask_piece_ends(reserve)), steps:
//   L<first>+<count>   one launch for masks [first, first + count)        E<i>   the event of piece i
//   C:<from>@<offset>><to>@<offset>#<bytes>                               a copy command; caller<i> / peer<i>: mask i's destination
#include "mask_transport.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace dlimg;

static std::string mem(MaskMem m, int mask) {
    switch (m) {
        case MaskMem::iou: return "iou";
        case MaskMem::device: return "device";
        case MaskMem::pinned: return "pinned";
        case MaskMem::caller: return "caller" + std::to_string(mask);
        default: return "peer" + std::to_string(mask);
    }
}

int main(int argc, char** argv) {
    MaskTransportPlan plan;
    if (argc >= 3 && !std::strcmp(argv[1], "device")) {
        std::vector<size_t> sizes;
        for (int i = 3; i < argc; ++i) sizes.push_back(std::strtoull(argv[i], nullptr, 10));
        plan_mask_transport_device(sizes, std::atoi(argv[2]) != 0, plan);
    } else if (argc >= 5 && !std::strcmp(argv[1], "host")) {
        MaskTransportInput in;
        in.direct_allowed = std::atoi(argv[2]) != 0;
        in.others_idle = std::atoi(argv[3]) != 0;
        in.iou_count = std::atoi(argv[4]);
        for (int i = 5; i < argc; ++i) {
            char* colon = nullptr;
            in.sizes.push_back(std::strtoull(argv[i], &colon, 10));
            in.dst_pinned.push_back(*colon == ':' && std::atoi(colon + 1) != 0);
        }
        plan_mask_transport(in, plan);
    } else {
        std::fprintf(stderr, "usage: %s host <direct_allowed> <others_idle> <iou_count> [bytes:pinned]... | device <kernel_writes_dst> [bytes]...\n", argv[0]);
        return 2;
    }
    const char* modes[] = {"none", "direct", "staged", "device_direct", "device_staged"};
    std::printf("mode %s\nlaunches %d\nkernel_dst", modes[(int)plan.mode], plan.launches);
    for (size_t d : plan.kernel_dst) d == kCallersPointer ? std::printf(" caller") : std::printf(" %zu", d);
    std::printf("\nin_place");
    for (char c : plan.in_place) std::printf(" %d", (int)c);
    std::printf("\npiece_end");
    for (size_t e : plan.piece_end) std::printf(" %zu", e);
    std::printf("\niou_offset %zu\nreserve %zu %zu\n", plan.iou_offset, plan.reserve_device, plan.reserve_pinned);
    std::printf("pieces_agree %d\nsteps", (int)(plan.piece_end == mask_piece_ends(plan.reserve_pinned)));
    for (MaskStep const& s : plan.steps) {
        if (s.kind == MaskStep::launch) std::printf(" L%d+%d", s.first, s.count);
        else if (s.kind == MaskStep::event) std::printf(" E%d", s.first);
        else std::printf(" C:%s@%zu>%s@%zu#%zu", mem(s.from, s.mask).c_str(), s.from_offset, mem(s.to, s.mask).c_str(), s.to_offset, s.bytes);
    }
    std::printf("\n");
    return 0;
}
