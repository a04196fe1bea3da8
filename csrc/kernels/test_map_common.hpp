// What the stand-alone CPU walks of the kernel maps (test_*_map.cpp) share: the CHECK macro, the failure
// counter and the final report.  A failed check prints
//   FAIL <subject>: <message> (<condition>, line <n>)
// and the walk goes on, so one run shows every broken invariant, up to 20 of them.  The subject is
// MAP_TEST_SUBJECT where the program defines it before this header (an expression in scope at every
// CHECK, such as the case's name), else the source file.  tests/test_kernel_maps_cpu.py builds the
// programs with -fsanitize=address,undefined and wants exit status 0 and a first line "OK ...".
#pragma once
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

#ifndef MAP_TEST_SUBJECT
#define MAP_TEST_SUBJECT __FILE__
#endif

namespace map_test {

inline int failures = 0;

__attribute__((format(printf, 4, 5))) inline void fail(const char* subject, const char* cond, int line,
                                                       const char* fmt, ...) {
  std::printf("FAIL %s", subject);
  va_list args;
  va_start(args, fmt);
  std::vprintf(fmt, args);
  va_end(args);
  std::printf(" (%s, line %d)\n", cond, line);
  if (++failures > 20) std::exit(1);
}

// The last statement of main: the program's "OK ..." line and 0, or the number of failures and 1.
__attribute__((format(printf, 1, 2))) inline int report(const char* ok_line, ...) {
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  va_list args;
  va_start(args, ok_line);
  std::vprintf(ok_line, args);
  va_end(args);
  return 0;
}

}  // namespace map_test

// CHECK(condition) or CHECK(condition, "printf format", arguments...)
#define CHECK(cond, ...)                                                                      \
  do {                                                                                        \
    if (!(cond)) map_test::fail(MAP_TEST_SUBJECT, #cond, __LINE__, ": " __VA_ARGS__);         \
  } while (0)
