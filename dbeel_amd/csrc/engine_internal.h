/* engine_internal.h — what dbeel_lsm.cpp calls in dbeel_gpu.hip beyond the
 * public ABI. Both files include it, so the compiler checks each definition
 * against the one prototype. Hidden: linked into the same library, not
 * exported. Internal to dbeel_amd/csrc; nothing here belongs to include/. */
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/dbeel_gpu.h"

#define DBEEL_HIDDEN __attribute__((visibility("hidden")))

extern "C" {
/* Sets the text dbeel_gpu_last_error returns on this thread. */
DBEEL_HIDDEN void dbeel_set_last_error(const char* msg);
/* Data bytes of the reader's run at pos; 0 when there is none. */
DBEEL_HIDDEN uint64_t dbeel_reader_run_data_len(const dbeel_gpu_reader* rd,
                                                size_t pos);
/* Takes the table at pos out of the reader's list again (a flush whose
 * files could not be written). */
DBEEL_HIDDEN int dbeel_reader_drop_run(dbeel_gpu_reader* rd, size_t pos);
}
