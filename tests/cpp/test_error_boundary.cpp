// The error model of the C boundary (coffeedb_amd/csrc/errors.h) on the host alone: the status is a property of the thrown error,
// never of its text.  Every case throws, is caught by catch (...) and goes through classify_current_exception(), as the guard of
// every C entry point does.
#include <cstdio>
#include <exception>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>

#include "errors.h"

using namespace cdb;

static int failures = 0;

template <typename Throw>
static void expect(const char* what, Throw&& thrower, int code, const std::string& message) {
    Failure f{0, ""};
    try {
        thrower();
    } catch (...) {
        f = classify_current_exception();
    }
    if (f.code != code || f.message != message) {
        std::printf("FAIL %s: got (%d, \"%s\"), want (%d, \"%s\")\n", what, f.code, f.message.c_str(), code, message.c_str());
        ++failures;
    }
}

int main() {
    constexpr int INVALID = 1, DEVICE = 2, INTERNAL = 3;  // CDB_E_* (include/coffeedb_gpu.h)
    static_assert((int)Status::Invalid == INVALID && (int)Status::Device == DEVICE && (int)Status::Internal == INTERNAL, "status values");

    expect("Error(msg)", [] { throw Error("x"); }, INVALID, "x");
    expect("Error(Invalid)", [] { throw Error(Status::Invalid, "a"); }, INVALID, "a");
    expect("Error(Device)", [] { throw Error(Status::Device, "b"); }, DEVICE, "b");
    expect("Error(Internal)", [] { throw Error(Status::Internal, "c"); }, INTERNAL, "c");
    expect("DeviceError", [] { throw DeviceError("d"); }, DEVICE, "d");
    expect("InternalError", [] { throw InternalError("e"); }, INTERNAL, "e");
    expect("LookbackTimeout as Error", [] {
        try {
            throw LookbackTimeout("radix sort look-back timed out (internal error)");
        } catch (const Error& e) {  // (by type: nothing reads the text)
            if (e.status != Status::Internal) throw std::logic_error("LookbackTimeout lost its status");
            throw;
        }
    }, INTERNAL, "radix sort look-back timed out (internal error)");
    expect("bad_alloc", [] { throw std::bad_alloc(); }, DEVICE, "out of host memory");
    expect("logic_error", [] { throw std::logic_error("y"); }, INTERNAL, "y");
    // text that the former substring rule misread: a caller's words echoed in the message
    expect("echoed \"internal\"", [] { throw Error("Invalid query: \"internal\""); }, INVALID, "Invalid query: \"internal\"");
    expect("echoed \"HIP error\"", [] { throw Error("HIP error [1,2] is no range"); }, INVALID, "HIP error [1,2] is no range");
    // a helper thread hands the error itself to the thread that joins it, not its text
    expect("Internal across a thread", [] {
        std::exception_ptr failure;
        std::thread t([&] {
            try {
                throw InternalError("the caller is not to blame");
            } catch (...) {
                failure = std::current_exception();
            }
        });
        t.join();
        if (failure) std::rethrow_exception(failure);
    }, INTERNAL, "the caller is not to blame");
    expect("bad_alloc across a thread", [] {
        std::exception_ptr failure;
        std::thread t([&] {
            try {
                throw std::bad_alloc();
            } catch (...) {
                failure = std::current_exception();
            }
        });
        t.join();
        if (failure) std::rethrow_exception(failure);
    }, DEVICE, "out of host memory");

    if (failures) return 1;
    std::printf("OK\n");
    return 0;
}
