// Stand-in for <boost/serialization/list.hpp> (TEST INFRASTRUCTURE): the reference's KeyFrameDatabase.h includes it for a
// serialize() member template that is never instantiated here.
#pragma once
