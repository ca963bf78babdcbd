// args_main_common.h -- TEST-ONLY.  What the stand-alone refusal programs (tests/bfv_*_args_main.cpp) share: a case is a statement that must
// throw std::invalid_argument (BAD) or must not (GOOD); one that goes the other way is printed with its group, its line and the reason, and
// counted in `failures`, which main() turns into the exit status.
#pragma once
#include <cstdio>
#include <stdexcept>
#include <string>

static int failures = 0;
template <class F> static void expect(bool refuse, const char *what, int k, F &&f) // k: the line of the case
{
    std::string why;
    bool refused = false;
    try {
        f();
    } catch (const std::invalid_argument &e) {
        refused = true;
        why = e.what();
    }
    if (refused != refuse) {
        std::printf("%s, line %d: %s %s\n", what, k, refuse ? "accepted, must be refused" : "refused, must be accepted:", why.c_str());
        ++failures;
    }
}
#define BAD(what, ...) expect(true, what, __LINE__, [&] { __VA_ARGS__; })
#define GOOD(what, ...) expect(false, what, __LINE__, [&] { __VA_ARGS__; })
