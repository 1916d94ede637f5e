// sw_abi_ptr.h — owners for the C ABI's objects (sw_amd.h) on the C++ side:
// std::unique_ptr with the object's own free function, so an early return or
// an exception frees what was made.
#ifndef SW_ABI_PTR_H
#define SW_ABI_PTR_H

#include <memory>

#include "sw_amd.h"

template <class T, int (*Free)(T*)>
struct sw_abi_free {
    void operator()(T* p) const { Free(p); }
};
typedef std::unique_ptr<sw_handle, sw_abi_free<sw_handle, sw_destroy> > sw_handle_ptr;
typedef std::unique_ptr<sw_db, sw_abi_free<sw_db, sw_db_free> > sw_db_ptr;
typedef std::unique_ptr<sw_pssm, sw_abi_free<sw_pssm, sw_pssm_free> > sw_pssm_ptr;
typedef std::unique_ptr<sw_group, sw_abi_free<sw_group, sw_group_destroy> > sw_group_ptr;
typedef std::unique_ptr<sw_gdb, sw_abi_free<sw_gdb, sw_group_db_free> > sw_gdb_ptr;

#endif  // SW_ABI_PTR_H
