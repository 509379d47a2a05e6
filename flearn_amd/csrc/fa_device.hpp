// fa_device.hpp — device code of the FedAVG-family aggregation engine (gfx950): the umbrella over
// the per-family headers.  Every kernel in them is one the product launches; each product unit
// includes only the families it launches, and the tuning tools include this file through
// tools/fa_tune_device.hpp, which adds the kernels only they launch.  Everything is header-only
// templates in namespace fa, except the few plain kernels of fa_segrows.hpp and fa_transport.hpp.
#pragma once

#include "fa_numerics.hpp"
#include "fa_stack.hpp"
#include "fa_segrows.hpp"
#include "fa_half.hpp"
#include "fa_fold.hpp"
#include "fa_trim.hpp"
#include "fa_gram.hpp"
#include "fa_transport.hpp"
