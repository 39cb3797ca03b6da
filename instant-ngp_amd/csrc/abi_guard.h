// abi_guard.h — what every C-ABI entry point wraps its body in: exceptions and bad arguments become the thread-local
// error string (ngp_last_error) and a return code. The string itself lives in engine_model.hip.
#pragma once
#include <exception>

#include "../../include/ngp_engine.h"
#include "common.h"

namespace ngp {
void set_last_error(const char* msg);
inline void check_rc(int rc) { if (rc != NGP_OK) throw Error(ngp_last_error()); }
inline hipStream_t S(void* s) { return (hipStream_t)s; }
}  // namespace ngp

#define NGP_TRY(...)                        \
	try {                                   \
		__VA_ARGS__;                        \
		return NGP_OK;                      \
	} catch (const std::exception& e) {     \
		::ngp::set_last_error(e.what());    \
		return NGP_ERROR;                   \
	}

#define NGP_ARG(cond)                                                                            \
	do {                                                                                         \
		if (!(cond)) { ::ngp::set_last_error("invalid argument: " #cond); return NGP_INVALID; } \
	} while (0)
