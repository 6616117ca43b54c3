// mgc_clock.hpp -- the host files' clock: seconds, monotonic
#pragma once
#include <chrono>
namespace mgc { inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); } }
