// tests/cpp/boost_standin/boost/shared_ptr.hpp -- a stand-in with the interface
// of boost::shared_ptr that the drop-in's md5(stream pointer) template relies on
// (copyable, const operator-> and operator* yielding a non-const T, get(), bool
// conversion), for tests/test_abi.py on a machine without Boost's headers.  Where
// the real Boost 1.49 headers are found, the test compiles against those instead.
#pragma once
#include <memory>

namespace boost {

template <class T>
class shared_ptr {
 public:
  shared_ptr() {}
  template <class Y>
  explicit shared_ptr(Y* p) : p_(p) {}
  template <class Y>
  shared_ptr(const shared_ptr<Y>& o) : p_(o.p_) {}

  T* get() const { return p_.get(); }
  T& operator*() const { return *p_; }
  T* operator->() const { return p_.get(); }
  explicit operator bool() const { return static_cast<bool>(p_); }
  void reset() { p_.reset(); }
  long use_count() const { return p_.use_count(); }

 private:
  template <class Y>
  friend class shared_ptr;
  std::shared_ptr<T> p_;
};

}  // namespace boost
