// errors.h — the library's error type and the one rule that turns an exception into a status code and a message.
// Standard headers only: a plain host program can include it (tests/cpp/test_error_boundary.cpp).
#pragma once
#include <exception>
#include <new>
#include <stdexcept>
#include <string>

namespace cdb {

// the CDB_E_* codes of include/coffeedb_gpu.h (capi.hip pins the values to them)
enum class Status : int { Invalid = 1, Device = 2, Internal = 3 };

// An error knows its status where it is thrown; its text is for people and decides nothing.  Error(msg) is the caller's
// mistake (Invalid); DeviceError = the GPU or its runtime failed; InternalError = a bug or a limit of the library itself.
struct Error : std::runtime_error {
    Status status;
    explicit Error(const std::string& msg) : std::runtime_error(msg), status(Status::Invalid) {}
    Error(Status st, const std::string& msg) : std::runtime_error(msg), status(st) {}
};
struct DeviceError : Error {
    explicit DeviceError(const std::string& msg) : Error(Status::Device, msg) {}
};
struct InternalError : Error {
    explicit InternalError(const std::string& msg) : Error(Status::Internal, msg) {}
};
// a look-back spin of the radix sort hit its bound (radix_sort.h: radix_check_error): build_suffix_array redoes the build in
// plain ticket order
struct LookbackTimeout : InternalError {
    using InternalError::InternalError;
};

struct Failure {
    int code;
    std::string message;
};
// What the C ABI reports for the exception in flight: call it inside a catch (...).
inline Failure classify_current_exception() {
    try {
        throw;
    } catch (const Error& e) {
        return {(int)e.status, e.what()};
    } catch (const std::bad_alloc&) {
        return {(int)Status::Device, "out of host memory"};
    } catch (const std::exception& e) {
        return {(int)Status::Internal, e.what()};
    }
}

}  // namespace cdb
