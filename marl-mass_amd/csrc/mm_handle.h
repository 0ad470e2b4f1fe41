// mm_handle.h -- the part of the library's handle that translation units outside the step library read.
//
// struct MMHandle_ (mm_step_host.h) derives from MMHandleHead; other translation units (mm_supervisor.hip) never see the
// full struct and reach these members only through mm_handle_head().
#pragma once
#include <stdint.h>

#include "../../include/mm_abi.h"

struct MMHandleHead {
  MMConfig cfg;
  int E, N, device;
  unsigned char *state;
  MMStateLayout lay;
  long long first_env;
};

// defined in mm_main.hip; not exported from the shared library
__attribute__((visibility("hidden"))) const MMHandleHead *mm_handle_head(MMHandle h);

// sets the text that mm_last_error(NULL) returns on this thread: how an entry point without a handle (mm_opt_step) says why it
// refused.  Defined in mm_main.hip; not exported from the shared library
__attribute__((visibility("hidden"))) void mm_set_thread_error(const char *text);
