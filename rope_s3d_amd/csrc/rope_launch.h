// rope_launch.h — host only: the one place where a launch function's run-time loss becomes a template argument.
#pragma once
#include <type_traits>

#include "rope_kernels.h"

namespace rope {

constexpr unsigned loss_bit(int loss) { return 1u << loss; }
constexpr unsigned LOSSES_ALL = 2 * loss_bit(ROPE_LOSS_CAMFULL) - 1;                          // ROPE_LOSS_DEPTH .. ROPE_LOSS_CAMFULL, the last
constexpr unsigned LOSSES_LAYERED = LOSSES_ALL & ~loss_bit(ROPE_LOSS_CAMFULL);      // the camera-pose loss has no shared layers

// f(std::integral_constant<int, ROPE_LOSS_x>{}) for the run-time `loss` if ALLOWED (bits loss_bit(ROPE_LOSS_x)) has it; -> whether f
// was called.  f is instantiated for the losses in ALLOWED only: a loss left out costs no kernel.
template <unsigned ALLOWED, class F>
static inline bool with_loss(int loss, F &&f)
{
    bool called = false;
    auto one = [&](auto l) {
        if constexpr ((ALLOWED & loss_bit(decltype(l)::value)) != 0)
            if (loss == decltype(l)::value) { f(l); called = true; }
    };
    one(std::integral_constant<int, ROPE_LOSS_DEPTH>{});
    one(std::integral_constant<int, ROPE_LOSS_FULL>{});
    one(std::integral_constant<int, ROPE_LOSS_LOOKUP>{});
    one(std::integral_constant<int, ROPE_LOSS_TSWEEP>{});
    one(std::integral_constant<int, ROPE_LOSS_CAMFULL>{});
    return called;
}

}  // namespace rope
